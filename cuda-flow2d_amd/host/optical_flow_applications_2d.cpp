// The applications built on the flow: frame interpolation, point trajectories, global motion and stabilisation, motion
// segmentation, deformation analysis, flow refinement and temporal denoising, and window correlation, which stands beside it.  Each has a
// ...Device entry on planes that already sit on the device
// and a host-image entry that uploads, calls it and downloads (CallPlanes + HostCall, host_entry.h).  The flow itself -- the
// pyramid, the sequence cache, ComputeFlow* -- is optical_flow_2d.cpp.
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "host_entry.h"
#include "optical_flow_2d.h"

bool OpticalFlow2D::InterpolationArgsOk(const float* times, size_t time_count, int iterations, float max_residual)
{
    if (!times || time_count == 0) return false;
    for (size_t j = 0; j < time_count; ++j)
        if (!(std::isfinite(times[j]) && times[j] >= 0.f && times[j] <= 1.f)) {
            std::printf("Error: '%s': interpolation time %g (0 <= t <= 1).\n", GetName(), times[j]);
            return false;
        }
    if (iterations < 1 || iterations > 16 || !std::isfinite(max_residual) || max_residual < 0.f) {
        std::printf("Error: '%s': interpolation iterations %d (1 .. 16) / max residual %g (finite, >= 0).\n", GetName(),
                    iterations, max_residual);
        return false;
    }
    return true;
}

bool OpticalFlow2D::QueueInterpolation(DevicePtr frame_0, DevicePtr frame_1, const DevicePtr* flows, bool use_masks,
                                       const float* times, size_t time_count, const DevicePtr* outputs, int iterations,
                                       float max_residual)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    for (size_t j = 0; j < time_count; ++j)
        if (CheckFlow2DError(flow2d_interpolate_2d(context_, AsPlane(frame_0), AsPlane(frame_1), AsPlane(flows[0]), AsPlane(flows[1]),
                                                   AsPlane(flows[2]), AsPlane(flows[3]), use_masks ? AsPlane(flows[4]) : nullptr,
                                                   use_masks ? AsPlane(flows[5]) : nullptr, W, H, pitch, times[j], iterations,
                                                   max_residual, AsPlane(outputs[j])),
                             "flow2d_interpolate_2d"))
            return false;
    return true;
}

bool OpticalFlow2D::InterpolateFramesDevice(const DevicePtr* dev_frames, size_t frame_count, const float* times, size_t time_count,
                                            const DevicePtr* dev_outputs, int iterations, float max_residual, bool use_masks,
                                            OperationParameters& params)
{
    if (!IsInitialized() || !dev_frames || !dev_outputs || frame_count < 2) return false;
    if (RefuseGroup("sequences")) return false;
    if (!InterpolationArgsOk(times, time_count, iterations, max_residual)) return false;
    // every output must be distinct from every other one and from the frames (which are only read)
    if (!WrittenPlanesOk(dev_frames, frame_count, dev_outputs, (frame_count - 1) * time_count, "output plane")) return false;
    if (!EnsurePlanes(interpolation_planes_, 6)) return false;
    const DevicePtr* p = interpolation_planes_.data();  // u, v, back u, back v, occlusion 0, occlusion 1
    bool ok = true;
    for (size_t k = 0; ok && k + 1 < frame_count; ++k) {
        ok = ComputeFlowBidirectionalDevice(dev_frames + k, 2, p, p + 1, p + 2, p + 3, use_masks ? p + 4 : nullptr,
                                            use_masks ? p + 5 : nullptr, params) &&
             QueueInterpolation(dev_frames[k], dev_frames[k + 1], p, use_masks, times, time_count, dev_outputs + k * time_count,
                                iterations, max_residual);
    }
    return ok;
}

void OpticalFlow2D::InterpolateFrames(Data2D& frame_0, Data2D& frame_1, const float* times, size_t time_count, Data2D* outputs,
                                      int iterations, float max_residual, bool use_masks, OperationParameters& params,
                                      Data2D* flow_u, Data2D* flow_v, Data2D* back_u, Data2D* back_v, Data2D* occlusion_0,
                                      Data2D* occlusion_1)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !outputs) return;
    if (RefuseGroup("sequences")) return;
    if (!InterpolationArgsOk(times, time_count, iterations, max_residual)) return;
    const size_t H = dev_container_size_.height;
    Data2D* flows[6] = {flow_u, flow_v, back_u, back_v, use_masks ? occlusion_0 : nullptr, use_masks ? occlusion_1 : nullptr};
    std::vector<Data2D*> images = {&frame_0, &frame_1};
    for (size_t j = 0; j < time_count; ++j) images.push_back(outputs + j);
    for (Data2D* d : flows)
        if (d) images.push_back(d);
    if (!SizeCheck{dev_container_size_, GetName(), "frame / output"}(images.data(), images.size())) return;
    if (!EnsurePlanes(bidirectional_planes_, 2) || !EnsurePlanes(interpolation_planes_, 6) ||
        !EnsurePlanes(interpolation_outputs_, time_count))
        return;
    HostCall call(context_, last_total_ms_);
    const size_t pitch = dev_container_size_.pitch;
    const DevicePtr* f = bidirectional_planes_.data();  // frame 0, frame 1
    bool ok = CopyData2DtoDevice(frame_0, f[0], H, pitch) && CopyData2DtoDevice(frame_1, f[1], H, pitch) &&
              InterpolateFramesDevice(f, 2, times, time_count, interpolation_outputs_.data(), iterations, max_residual, use_masks,
                                      params);
    for (size_t j = 0; ok && j < time_count; ++j) ok = CopyData2DFromDevice(interpolation_outputs_[j], outputs[j], H, pitch);
    for (int i = 0; ok && i < 6; ++i)
        if (flows[i]) ok = CopyData2DFromDevice(interpolation_planes_[i], *flows[i], H, pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::TrackPointsDevice(const DevicePtr* dev_frames, size_t frame_count, size_t spacing, float min_eigenvalue,
                                      bool check_boundaries, float beta1, float beta2, const DevicePtr* dev_xs,
                                      const DevicePtr* dev_ys, size_t capacity, unsigned long long* counts_out,
                                      OperationParameters& params)
{
    if (!IsInitialized() || !dev_frames || !dev_xs || !dev_ys || !counts_out || frame_count < 2 || capacity == 0) return false;
    if (RefuseGroup("sequences")) return false;
    if (spacing == 0 || !(std::isfinite(min_eigenvalue) && min_eigenvalue >= 0.f) ||
        !(std::isfinite(beta1) && beta1 >= 0.f && std::isfinite(beta2) && beta2 >= 0.f)) {
        std::printf("Error: '%s': tracking spacing %zu (>= 1), min eigenvalue %g, boundary thresholds %g / %g (finite, >= 0).\n",
                    GetName(), spacing, min_eigenvalue, beta1, beta2);
        return false;
    }
    float alpha1 = 0.01f, alpha2 = 0.5f;  // Sundaram, Brox & Keutzer (ECCV 2010)
    params.Read<float>("consistency_alpha1", alpha1);
    params.Read<float>("consistency_alpha2", alpha2);
    if (!(std::isfinite(alpha1) && std::isfinite(alpha2) && alpha1 >= 0.f && alpha2 >= 0.f)) {
        std::printf("Error: '%s': consistency thresholds %g / %g (finite, >= 0).\n", GetName(), alpha1, alpha2);
        return false;
    }
    // every table is written: distinct from each other and from the frames
    std::vector<DevicePtr> tables(dev_xs, dev_xs + frame_count);
    tables.insert(tables.end(), dev_ys, dev_ys + frame_count);
    if (!WrittenPlanesOk(dev_frames, frame_count, tables.data(), tables.size(), "track table")) return false;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const size_t window = std::min(kTrackWindow, frame_count - 1);
    if (!EnsurePlanes(tracking_flows_, 4 * window)) return false;
    // the device count (16 bytes) and the seeding workspace behind it
    const size_t workspace_bytes = flow2d_seed_points_workspace_bytes(W, H, spacing);
    if (!tracking_scratch_.Ensure(context_, 16 + workspace_bytes)) return false;
    unsigned long long* dev_count = tracking_scratch_.At<unsigned long long>();
    void* workspace = tracking_scratch_.At(16);
    void* host_counts = nullptr;  // page-locked: the per-frame counts are copied into it on the stream
    if (CheckFlow2DError(flow2d_host_alloc(context_, frame_count * sizeof(unsigned long long), &host_counts), "flow2d_host_alloc"))
        return false;
    unsigned long long* counts = static_cast<unsigned long long*>(host_counts);
    const size_t table_bytes = capacity * sizeof(float);
    auto seed = [&](size_t k) {
        return !CheckFlow2DError(flow2d_seed_points_2d(context_, AsPlane(dev_frames[k]), W, H, pitch, spacing, min_eigenvalue,
                                                       AsPlane(dev_xs[k]), AsPlane(dev_ys[k]), dev_count, capacity, nullptr,
                                                       workspace, workspace_bytes),
                                 "flow2d_seed_points_2d") &&
               ReadRecord(counts + k, dev_count, sizeof(unsigned long long));
    };
    // table 0: no track yet (all NaN: 0xff bytes), count 0, then the initial seeding
    bool ok = !CheckFlow2DError(flow2d_memset_2d(context_, AsPlane(dev_xs[0]), table_bytes, 0xff, table_bytes, 1), "flow2d_memset_2d") &&
              !CheckFlow2DError(flow2d_memset_2d(context_, AsPlane(dev_ys[0]), table_bytes, 0xff, table_bytes, 1), "flow2d_memset_2d") &&
              !CheckFlow2DError(flow2d_memset_2d(context_, dev_count, 16, 0, 16, 1), "flow2d_memset_2d") && seed(0);
    const DevicePtr* f = tracking_flows_.data();  // pair j of a window: u, v, back u, back v at 4 j
    for (size_t start = 0; ok && start + 1 < frame_count; start += window) {
        const size_t pairs = std::min(window, frame_count - 1 - start);
        std::vector<DevicePtr> us(pairs), vs(pairs), bus(pairs), bvs(pairs);
        for (size_t j = 0; j < pairs; ++j) {
            us[j] = f[4 * j];
            vs[j] = f[4 * j + 1];
            bus[j] = f[4 * j + 2];
            bvs[j] = f[4 * j + 3];
        }
        ok = ComputeFlowBidirectionalDevice(dev_frames + start, pairs + 1, us.data(), vs.data(), bus.data(), bvs.data(), nullptr,
                                            nullptr, params);
        for (size_t j = 0; ok && j < pairs; ++j) {
            const size_t k = start + j;
            ok = !CheckFlow2DError(flow2d_track_points_2d(context_, AsPlane(us[j]), AsPlane(vs[j]), AsPlane(bus[j]), AsPlane(bvs[j]),
                                                          W, H, pitch, AsPlane(dev_xs[k]), AsPlane(dev_ys[k]), dev_count,
                                                          capacity, alpha1, alpha2, check_boundaries ? 1 : 0, beta1, beta2,
                                                          AsPlane(dev_xs[k + 1]), AsPlane(dev_ys[k + 1]), nullptr),
                                   "flow2d_track_points_2d") &&
                 seed(k + 1);
        }
    }
    ok = !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;  // the only host wait
    if (ok)
        for (size_t k = 0; k < frame_count; ++k) counts_out[k] = counts[k];
    flow2d_host_free(context_, host_counts);
    return ok;
}

void OpticalFlow2D::TrackPoints(Data2D* const* frames, size_t frame_count, size_t spacing, float min_eigenvalue,
                                bool check_boundaries, float beta1, float beta2, float* xs, float* ys, size_t capacity,
                                unsigned long long* counts_out, OperationParameters& params)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !frames || !xs || !ys || !counts_out || frame_count < 2 || capacity == 0) return;
    if (RefuseGroup("sequences")) return;
    // the planes of this call: the frames, then the x tables, then the y tables
    const size_t n = frame_count, table_bytes = capacity * sizeof(float);
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame");
    planes.Add(frames, n, CallPlanes::In).AddBytes(table_bytes, 2 * n);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr *d = planes.data(), *dev_xs = d + n, *dev_ys = d + 2 * n;
    bool ok = planes.Upload() && TrackPointsDevice(d, n, spacing, min_eigenvalue, check_boundaries, beta1, beta2, dev_xs, dev_ys,
                                                   capacity, counts_out, params);
    for (size_t k = 0; ok && k < n; ++k)
        ok = ReadRecord(xs + k * capacity, AsPlane(dev_xs[k]), table_bytes) && ReadRecord(ys + k * capacity, AsPlane(dev_ys[k]), table_bytes);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::GlobalMotionArgsOk(int model, double sigma, int iterations)
{
    if ((model != FLOW2D_MOTION_TRANSLATION && model != FLOW2D_MOTION_SIMILARITY && model != FLOW2D_MOTION_AFFINE) ||
        !std::isfinite(sigma) || sigma < 0.0 || iterations < 0 || iterations > FLOW2D_GLOBAL_MOTION_MAX_ITERATIONS) {
        std::printf("Error: global motion takes a model of 0 (translation), 1 (similarity) or 2 (affine) (%d), a finite sigma >= 0 (%g) "
                    "and 0 .. %d iterations (%d).\n",
                    model, sigma, FLOW2D_GLOBAL_MOTION_MAX_ITERATIONS, iterations);
        return false;
    }
    return true;
}

flow2d_global_motion OpticalFlow2D::ComposeGlobalMotion(const flow2d_global_motion& first, const flow2d_global_motion& second)
{
    const double a1[4] = {1.0 + first.p[1], first.p[2], first.p[4], 1.0 + first.p[5]};
    const double a2[4] = {1.0 + second.p[1], second.p[2], second.p[4], 1.0 + second.p[5]};
    flow2d_global_motion out = second;  // weight_sum, support: the newest fit's
    const double a11 = a2[0] * a1[0] + a2[1] * a1[2], a12 = a2[0] * a1[1] + a2[1] * a1[3];
    const double a21 = a2[2] * a1[0] + a2[3] * a1[2], a22 = a2[2] * a1[1] + a2[3] * a1[3];
    out.p[0] = (a2[0] * first.p[0] + a2[1] * first.p[3]) + second.p[0];
    out.p[1] = a11 - 1.0;
    out.p[2] = a12;
    out.p[3] = (a2[2] * first.p[0] + a2[3] * first.p[3]) + second.p[3];
    out.p[4] = a21;
    out.p[5] = a22 - 1.0;
    out.model_used = std::max(first.model_used, second.model_used);
    return out;
}

bool OpticalFlow2D::EnsureStabiliseScratch()
{
    const size_t records = (kStabiliseWindow + 1) * sizeof(flow2d_global_motion);  // a multiple of 16
    return stabilise_scratch_.Ensure(context_, records + flow2d_global_motion_workspace_bytes(dev_container_size_.width,
                                                                                               dev_container_size_.height, 1));
}

bool OpticalFlow2D::FitConsecutivePairs(const DevicePtr* frames, size_t count, int model, double sigma, int iterations,
                                        bool use_masks, flow2d_global_motion* records, OperationParameters& params)
{
    if (count < 2) return true;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const size_t per_pair = use_masks ? 6 : 2;
    for (size_t j = 0; j < kStabiliseWindow; ++j)
        if (!EnsurePlanes(&stabilise_planes_[6 * j], per_pair)) return false;
    if (!EnsureStabiliseScratch()) return false;
    void* workspace = StabiliseRecord(kStabiliseWindow + 1);
    const size_t workspace_bytes = flow2d_global_motion_workspace_bytes(W, H, 1);
    bool ok = true;
    for (size_t start = 0; ok && start + 1 < count; start += kStabiliseWindow) {
        const size_t pairs = std::min(kStabiliseWindow, count - 1 - start);
        std::vector<DevicePtr> p[6];
        for (size_t j = 0; j < pairs; ++j)
            for (size_t i = 0; i < 6; ++i) p[i].push_back(stabilise_planes_[6 * j + i]);
        ok = use_masks ? ComputeFlowBidirectionalDevice(frames + start, pairs + 1, p[0].data(), p[1].data(), p[2].data(), p[3].data(),
                                                        p[4].data(), p[5].data(), params)
                       : ComputeFlowSequenceDevice(frames + start, pairs + 1, p[0].data(), p[1].data(), params);
        for (size_t j = 0; ok && j < pairs; ++j)
            ok = !CheckFlow2DError(flow2d_global_motion_2d(context_, AsPlane(p[0][j]), AsPlane(p[1][j]),
                                                           use_masks ? AsPlane(p[4][j]) : nullptr, W, H, pitch, model, sigma,
                                                           iterations, StabiliseRecord(j), workspace, workspace_bytes),
                                   "flow2d_global_motion_2d") &&
                 ReadRecord(records + start + j, StabiliseRecord(j), sizeof(flow2d_global_motion));
        // the records are read by the host next, and the window's planes and record slots are reused
        ok = !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
    }
    return ok;
}

bool OpticalFlow2D::EstimateGlobalMotionDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, int model, double sigma,
                                               int iterations, bool use_masks, flow2d_global_motion* motion_out,
                                               OperationParameters& params, DevicePtr dev_flow_u, DevicePtr dev_flow_v,
                                               DevicePtr dev_residual_u, DevicePtr dev_residual_v)
{
    if (!GlobalMotionArgsOk(model, sigma, iterations)) return false;
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || !motion_out) return false;
    if (RefuseGroup("global motion")) return false;
    if ((dev_flow_u == 0) != (dev_flow_v == 0) || (dev_residual_u == 0) != (dev_residual_v == 0)) return false;
    const DevicePtr frames[2] = {dev_frame_0, dev_frame_1};
    if (!FitConsecutivePairs(frames, 2, model, sigma, iterations, use_masks, motion_out, params)) return false;
    // the pair's flow and record are still in slot 0
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const DevicePtr flow[2] = {dev_flow_u, dev_flow_v};
    bool ok = HandBack(2, stabilise_planes_.data(), flow);
    if (ok && dev_residual_u)
        ok = !CheckFlow2DError(flow2d_global_flow_2d(context_, StabiliseRecord(0), AsPlane(stabilise_planes_[0]),
                                                     AsPlane(stabilise_planes_[1]), nullptr, W, H, pitch, 0.0, nullptr, nullptr,
                                                     AsPlane(dev_residual_u), AsPlane(dev_residual_v), nullptr),
                               "flow2d_global_flow_2d");
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::EstimateGlobalMotion(Data2D& frame_0, Data2D& frame_1, int model, double sigma, int iterations, bool use_masks,
                                         flow2d_global_motion* motion_out, OperationParameters& params, Data2D* flow_u,
                                         Data2D* flow_v, Data2D* residual_u, Data2D* residual_v)
{
    last_run_ok_ = false;
    if (!GlobalMotionArgsOk(model, sigma, iterations)) return;
    if (!IsInitialized() || !motion_out) return;
    // (the device entry is handed all four output planes, wanted or not)
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In);
    for (Data2D* image : {flow_u, flow_v, residual_u, residual_v}) planes.Add(image, CallPlanes::Out, true);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    last_run_ok_ = planes.Upload() &&
                   EstimateGlobalMotionDevice(d[0], d[1], model, sigma, iterations, use_masks, motion_out, params, d[2], d[3], d[4], d[5]) &&
                   planes.Download();
}

bool OpticalFlow2D::SegmentMotionArgsOk(float threshold, float join, unsigned min_area)
{
    if (!(threshold >= 0.f) || !(join >= 0.f) || min_area == 0) {
        std::printf("Error: motion segmentation takes a threshold >= 0 (%g), a join >= 0, infinity allowed (%g), and a min_area >= 1 (%u).\n",
                    threshold, join, min_area);
        return false;
    }
    return true;
}

bool OpticalFlow2D::SegmentMotionDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, int model, double sigma, int iterations,
                                        bool use_masks, float threshold, float join, unsigned min_area,
                                        flow2d_global_motion* motion_out, flow2d_segment_summary* summary_out,
                                        flow2d_motion_region* regions_out, OperationParameters& params, DevicePtr dev_labels,
                                        DevicePtr dev_residual_u, DevicePtr dev_residual_v)
{
    if (!GlobalMotionArgsOk(model, sigma, iterations) || !SegmentMotionArgsOk(threshold, join, min_area)) return false;
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || !motion_out || !summary_out) return false;
    if ((dev_residual_u == 0) != (dev_residual_v == 0)) return false;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    constexpr size_t kTableOffset = 64;  // the summary comes first
    const size_t table_bytes = kSegmentMaxRegions * sizeof(flow2d_motion_region);
    const size_t workspace_bytes = flow2d_segment_motion_workspace_bytes(W, H, 1);
    if (!EnsurePlanes(segment_planes_, 3)) return false;
    if (!segment_scratch_.Ensure(context_, kTableOffset + table_bytes + workspace_bytes)) return false;
    // the flow, the fit and the residual planes (group_ > 1 is refused there); with use_masks the forward occlusion mask of
    // the pair is still in the window's slot 0 afterwards
    if (!EstimateGlobalMotionDevice(dev_frame_0, dev_frame_1, model, sigma, iterations, use_masks, motion_out, params, 0, 0,
                                    segment_planes_[0], segment_planes_[1]))
        return false;
    flow2d_segment_summary* summary = segment_scratch_.At<flow2d_segment_summary>();
    flow2d_motion_region* table = segment_scratch_.At<flow2d_motion_region>(kTableOffset);
    bool ok = !CheckFlow2DError(
        flow2d_segment_motion_2d(context_, AsPlane(segment_planes_[0]), AsPlane(segment_planes_[1]),
                                 use_masks ? AsPlane(stabilise_planes_[4]) : nullptr, W, H, pitch, threshold, join, min_area,
                                 reinterpret_cast<int*>(AsPlane(segment_planes_[2])), table, kSegmentMaxRegions, summary,
                                 segment_scratch_.At(kTableOffset + table_bytes), workspace_bytes),
        "flow2d_segment_motion_2d");
    ok = ok && ReadRecord(summary_out, summary, sizeof(*summary_out)) && (!regions_out || ReadRecord(regions_out, table, table_bytes));
    const DevicePtr own[3] = {segment_planes_[2], segment_planes_[0], segment_planes_[1]};
    const DevicePtr callers[3] = {dev_labels, dev_residual_u, dev_residual_v};
    ok = ok && HandBack(1, own, callers) && HandBack(2, own + 1, callers + 1);
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::SegmentMotion(Data2D& frame_0, Data2D& frame_1, int model, double sigma, int iterations, bool use_masks,
                                  float threshold, float join, unsigned min_area, flow2d_global_motion* motion_out,
                                  flow2d_segment_summary* summary_out, flow2d_motion_region* regions_out,
                                  OperationParameters& params, Data2D* labels, Data2D* residual_u, Data2D* residual_v)
{
    last_run_ok_ = false;
    if (!GlobalMotionArgsOk(model, sigma, iterations) || !SegmentMotionArgsOk(threshold, join, min_area)) return;
    if (!IsInitialized() || !motion_out || !summary_out || (residual_u == nullptr) != (residual_v == nullptr)) return;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / labels / residual");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In);
    planes.Add(labels, CallPlanes::Out).Add(residual_u, CallPlanes::Out).Add(residual_v, CallPlanes::Out);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    last_run_ok_ = planes.Upload() &&
                   SegmentMotionDevice(d[0], d[1], model, sigma, iterations, use_masks, threshold, join, min_area, motion_out, summary_out,
                                       regions_out, params, d[2], d[3], d[4]) &&
                   planes.Download();
}

bool OpticalFlow2D::DeformationArgsOk(int measure, float smoothing_sigma)
{
    // (the blur runs with up to 51 taps, 3 sigma to each side: flow2d_gaussian_kernel)
    if ((measure != FLOW2D_STRAIN_SMALL && measure != FLOW2D_STRAIN_GREEN_LAGRANGE) || !(smoothing_sigma >= 0.f) ||
        !(smoothing_sigma < 26.f / 3.f)) {
        std::printf("Error: deformation analysis takes a strain measure 0 (small) or 1 (Green-Lagrange) (%d) and a smoothing sigma in [0, 8.66] (%g).\n",
                    measure, smoothing_sigma);
        return false;
    }
    return true;
}

bool OpticalFlow2D::AnalyseDeformationDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, int measure, float smoothing_sigma,
                                             bool use_masks, const DevicePtr* dev_planes, flow2d_deformation_stats* stats_out,
                                             OperationParameters& params, DevicePtr dev_flow_u, DevicePtr dev_flow_v,
                                             DevicePtr dev_mask)
{
    if (!DeformationArgsOk(measure, smoothing_sigma)) return false;
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || (dev_flow_u == 0) != (dev_flow_v == 0) || (dev_mask && !use_masks))
        return false;
    flow2d_deformation_planes out = {};
    float** slots[9] = {&out.divergence, &out.vorticity, &out.dilatation, &out.exx, &out.eyy, &out.exy, &out.e1, &out.e2, &out.max_shear};
    bool any = stats_out != nullptr;
    for (int k = 0; dev_planes && k < 9; ++k) {
        *slots[k] = AsPlane(dev_planes[k]);
        any = any || dev_planes[k];
    }
    if (!any) return false;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const bool smooth = smoothing_sigma > 0.f;
    DevicePtr* p = deformation_planes_.begin();
    if (!EnsurePlanes(p, use_masks ? 6 : 2) || (smooth && !EnsurePlanes(p + 6, 2))) return false;
    constexpr size_t kWorkspaceOffset = sizeof(flow2d_deformation_stats);  // the record comes first
    const size_t workspace_bytes = flow2d_deformation_workspace_bytes(W, H, 1);
    if (stats_out && !deformation_scratch_.Ensure(context_, kWorkspaceOffset + workspace_bytes)) return false;
    // (group_ > 1 is refused by both)
    const DevicePtr frames[2] = {dev_frame_0, dev_frame_1};
    if (!(use_masks ? ComputeFlowBidirectionalDevice(frames, 2, p, p + 1, p + 2, p + 3, p + 4, p + 5, params)
                    : ComputeFlowSequenceDevice(frames, 2, p, p + 1, params)))
        return false;
    bool ok = true;
    if (smooth) {
        float taps[51];
        int radius = 0;
        ok = !CheckFlow2DError(flow2d_gaussian_kernel(smoothing_sigma, taps, &radius), "flow2d_gaussian_kernel");
        for (int i = 0; ok && i < 2; ++i)
            ok = !CheckFlow2DError(flow2d_gaussian_blur(context_, AsPlane(p[6 + i]), AsPlane(p[i]), W, H, pitch, taps, radius),
                                   "flow2d_gaussian_blur");
    }
    const DevicePtr* flow = smooth ? p + 6 : p;
    flow2d_deformation_stats* record = stats_out ? deformation_scratch_.At<flow2d_deformation_stats>() : nullptr;
    ok = ok && !CheckFlow2DError(flow2d_deformation_2d(context_, AsPlane(flow[0]), AsPlane(flow[1]), use_masks ? AsPlane(p[4]) : nullptr,
                                                       W, H, pitch, measure, &out, record,
                                                       stats_out ? deformation_scratch_.At(kWorkspaceOffset) : nullptr, workspace_bytes),
                                 "flow2d_deformation_2d");
    ok = ok && (!stats_out || ReadRecord(stats_out, record, sizeof(*stats_out)));
    const DevicePtr own[3] = {flow[0], flow[1], p[4]}, callers[3] = {dev_flow_u, dev_flow_v, dev_mask};
    ok = ok && HandBack(2, own, callers) && HandBack(1, own + 2, callers + 2);
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::AnalyseDeformation(Data2D& frame_0, Data2D& frame_1, int measure, float smoothing_sigma, bool use_masks,
                                       Data2D* const* deformation, flow2d_deformation_stats* stats_out, OperationParameters& params,
                                       Data2D* flow_u, Data2D* flow_v, Data2D* mask)
{
    last_run_ok_ = false;
    if (!DeformationArgsOk(measure, smoothing_sigma)) return;
    if (!IsInitialized() || (flow_u == nullptr) != (flow_v == nullptr) || (mask && !use_masks)) return;
    // the planes of this call: only those that are asked for
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow / deformation");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In);
    planes.Add(flow_u, CallPlanes::Out).Add(flow_v, CallPlanes::Out).Add(mask, CallPlanes::Out).Add(deformation, 9, CallPlanes::Out);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    last_run_ok_ = planes.Upload() &&
                   AnalyseDeformationDevice(d[0], d[1], measure, smoothing_sigma, use_masks, d + 5, stats_out, params, d[2], d[3], d[4]) &&
                   planes.Download();
}

bool OpticalFlow2D::RefineArgsOk(int radius, float sigma_guide, float sigma_space, int iterations)
{
    if (radius < 1 || radius > FLOW2D_REFINE_MAX_RADIUS || !(std::isfinite(sigma_guide) && sigma_guide >= 0.f) ||
        !(std::isfinite(sigma_space) && sigma_space >= 0.f) || iterations < 1 || iterations > kRefineMaxIterations) {
        std::printf("Error: flow refinement takes a radius of 1 .. %d (%d), finite sigmas >= 0 (guide %g, space %g) and 1 .. %d iterations (%d).\n",
                    FLOW2D_REFINE_MAX_RADIUS, radius, sigma_guide, sigma_space, kRefineMaxIterations, iterations);
        return false;
    }
    return true;
}

bool OpticalFlow2D::RefineFlowDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, int radius, float sigma_guide, float sigma_space,
                                     int iterations, bool use_masks, DevicePtr dev_refined_u, DevicePtr dev_refined_v,
                                     flow2d_refine_record* record_out, OperationParameters& params, DevicePtr dev_flow_u,
                                     DevicePtr dev_flow_v, DevicePtr dev_mask, bool flow_given)
{
    if (!RefineArgsOk(radius, sigma_guide, sigma_space, iterations)) return false;
    if (!IsInitialized() || !dev_frame_0 || !dev_refined_u || !dev_refined_v || (dev_flow_u == 0) != (dev_flow_v == 0)) return false;
    if (flow_given ? !dev_flow_u : (!dev_frame_1 || (dev_mask && !use_masks))) return false;
    if (RefuseGroup("flow refinement")) return false;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    DevicePtr* p = refine_planes_.begin();
    const size_t middle = iterations > 2 ? 4 : iterations > 1 ? 2 : 0;  // ping-pong planes of the passes before the last
    if ((!flow_given && !EnsurePlanes(p, use_masks ? 6 : 2)) || !EnsurePlanes(p + 6, middle)) return false;
    if (record_out && !refine_scratch_.Ensure(context_, sizeof(flow2d_refine_record))) return false;
    DevicePtr flow[2] = {dev_flow_u, dev_flow_v}, mask = dev_mask;
    if (!flow_given) {
        // (group_ > 1 is refused by both)
        const DevicePtr frames[2] = {dev_frame_0, dev_frame_1};
        if (!(use_masks ? ComputeFlowBidirectionalDevice(frames, 2, p, p + 1, p + 2, p + 3, p + 4, p + 5, params)
                        : ComputeFlowSequenceDevice(frames, 2, p, p + 1, params)))
            return false;
        flow[0] = p[0];
        flow[1] = p[1];
        mask = use_masks ? p[4] : 0;
    }
    flow2d_refine_record* record = record_out ? refine_scratch_.At<flow2d_refine_record>() : nullptr;
    bool ok = true;
    const DevicePtr* in = flow;
    for (int k = 0; ok && k < iterations; ++k) {
        const bool last = k + 1 == iterations;
        const DevicePtr refined[2] = {dev_refined_u, dev_refined_v};
        const DevicePtr* out = last ? refined : p + 6 + 2 * (k % 2);
        ok = !CheckFlow2DError(flow2d_refine_flow_2d(context_, AsPlane(in[0]), AsPlane(in[1]), AsPlane(dev_frame_0),
                                                     mask ? AsPlane(mask) : nullptr, W, H, pitch, radius, sigma_guide, sigma_space,
                                                     AsPlane(out[0]), AsPlane(out[1]), last ? record : nullptr),
                               "flow2d_refine_flow_2d");
        in = p + 6 + 2 * (k % 2);
    }
    ok = ok && (!record_out || ReadRecord(record_out, record, sizeof(*record_out)));
    if (ok && !flow_given) {
        const DevicePtr own[3] = {flow[0], flow[1], mask}, callers[3] = {dev_flow_u, dev_flow_v, dev_mask};
        ok = HandBack(2, own, callers) && (!mask || HandBack(1, own + 2, callers + 2));
    }
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::RefineFlow(Data2D& frame_0, Data2D& frame_1, int radius, float sigma_guide, float sigma_space, int iterations,
                               bool use_masks, Data2D& refined_u, Data2D& refined_v, flow2d_refine_record* record_out,
                               OperationParameters& params, Data2D* flow_u, Data2D* flow_v, Data2D* mask)
{
    last_run_ok_ = false;
    if (!RefineArgsOk(radius, sigma_guide, sigma_space, iterations)) return;
    if (!IsInitialized() || (flow_u == nullptr) != (flow_v == nullptr) || (mask && !use_masks)) return;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In).Add(&refined_u, CallPlanes::Out).Add(&refined_v, CallPlanes::Out);
    planes.Add(flow_u, CallPlanes::Out).Add(flow_v, CallPlanes::Out).Add(mask, CallPlanes::Out);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    last_run_ok_ = planes.Upload() &&
                   RefineFlowDevice(d[0], d[1], radius, sigma_guide, sigma_space, iterations, use_masks, d[2], d[3], record_out, params,
                                    d[4], d[5], d[6]) &&
                   planes.Download();
}

bool OpticalFlow2D::CorrelationArgsOk(size_t width, size_t height, float lo, float scale, int radius, int range, int spacing,
                                      float min_score)
{
    size_t nw = 0, nh = 0;
    if (radius < 1 || radius > FLOW2D_CORRELATION_MAX_RADIUS || range < 1 || range > FLOW2D_CORRELATION_MAX_RANGE || spacing < 1 ||
        spacing > FLOW2D_CORRELATION_MAX_SPACING || !(std::isfinite(scale) && scale > 0.f) || !std::isfinite(lo) || std::isnan(min_score)) {
        std::printf("Error: window correlation takes a radius of 1 .. %d (%d), a range of 1 .. %d (%d), a spacing of 1 .. %d (%d), a "
                    "finite lo (%g), a finite scale > 0 (%g) and a minimum score that is a number (%g).\n",
                    FLOW2D_CORRELATION_MAX_RADIUS, radius, FLOW2D_CORRELATION_MAX_RANGE, range, FLOW2D_CORRELATION_MAX_SPACING, spacing,
                    lo, scale, min_score);
        return false;
    }
    if (flow2d_correlation_grid(width, height, radius, spacing, &nw, &nh) != FLOW2D_OK) {
        std::printf("Error: a %zu x %zu frame is smaller than one correlation window of radius %d.\n", width, height, radius);
        return false;
    }
    return true;
}

bool OpticalFlow2D::CorrelateDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, int radius, int range,
                                    int spacing, float min_score, DevicePtr dev_node_u, DevicePtr dev_node_v, DevicePtr dev_node_score,
                                    flow2d_correlation_record* record_out, DevicePtr dev_flow_u, DevicePtr dev_flow_v)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!CorrelationArgsOk(W, H, lo, scale, radius, range, spacing, min_score)) return false;
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || (dev_flow_u == 0) != (dev_flow_v == 0)) return false;
    if (RefuseGroup("window correlation")) return false;
    DevicePtr* own = correlation_planes_.begin();
    DevicePtr node[2] = {dev_node_u, dev_node_v};
    for (int k = 0; k < 2; ++k) {
        if (node[k]) continue;
        if (!EnsurePlanes(own + k, 1)) return false;
        node[k] = own[k];
    }
    if (record_out && !correlation_scratch_.Ensure(context_, sizeof(flow2d_correlation_record))) return false;
    flow2d_correlation_record* record = record_out ? correlation_scratch_.At<flow2d_correlation_record>() : nullptr;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(W, H, radius, spacing, &nw, &nh);
    // (the node planes are containers: the frames' pitch)
    bool ok = !CheckFlow2DError(flow2d_correlate_2d(context_, AsPlane(dev_frame_0), AsPlane(dev_frame_1), W, H, pitch, lo, scale, radius,
                                                    range, spacing, min_score, AsPlane(node[0]), AsPlane(node[1]),
                                                    dev_node_score ? AsPlane(dev_node_score) : nullptr, pitch, record),
                                "flow2d_correlate_2d");
    if (ok && dev_flow_u)
        ok = !CheckFlow2DError(flow2d_expand_nodes_2d(context_, AsPlane(node[0]), AsPlane(node[1]), nw, nh, pitch, radius, spacing,
                                                      AsPlane(dev_flow_u), AsPlane(dev_flow_v), W, H, pitch),
                               "flow2d_expand_nodes_2d");
    ok = ok && (!record_out || ReadRecord(record_out, record, sizeof(*record_out)));
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::CorrelationRange(Data2D& frame_0, Data2D& frame_1, float& lo, float& scale)
{
    float low = INFINITY, high = -INFINITY;
    for (Data2D* image : {&frame_0, &frame_1}) {
        const float* p = image->DataPtr();
        const size_t n = image->Width() * image->Height();
        for (size_t i = 0; i < n; ++i) {
            if (!std::isfinite(p[i])) continue;
            low = std::min(low, p[i]);
            high = std::max(high, p[i]);
        }
    }
    lo = 0.f;
    scale = 1.f;
    if (!(low <= high) || (low >= 0.f && high <= 255.f) || !(high - low > 0.f)) return;  // nothing finite, 8-bit data, or flat
    lo = low;
    scale = 255.f / (high - low);
}

void OpticalFlow2D::Correlate(Data2D& frame_0, Data2D& frame_1, int radius, int range, int spacing, float min_score, Data2D& node_u,
                              Data2D& node_v, Data2D* node_score, flow2d_correlation_record* record_out, Data2D* flow_u, Data2D* flow_v)
{
    last_run_ok_ = false;
    if (!IsInitialized() || (flow_u == nullptr) != (flow_v == nullptr)) return;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In).Add(flow_u, CallPlanes::Out).Add(flow_v, CallPlanes::Out);
    // the node planes: containers with no image of their size behind them, downloaded below
    planes.Add(nullptr, CallPlanes::Out, true).Add(nullptr, CallPlanes::Out, true).Add(nullptr, CallPlanes::Out, node_score != nullptr);
    if (!planes.SizesMatch()) return;
    float lo = 0.f, scale = 1.f;
    CorrelationRange(frame_0, frame_1, lo, scale);
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    if (!CorrelationArgsOk(W, H, lo, scale, radius, range, spacing, min_score)) return;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(W, H, radius, spacing, &nw, &nh);
    Data2D* nodes[3] = {&node_u, &node_v, node_score};
    for (Data2D* image : nodes)
        if (image && (image->Width() != nw || image->Height() != nh)) {
            std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
            return;
        }
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    bool ok = planes.Upload() &&
              CorrelateDevice(d[0], d[1], lo, scale, radius, range, spacing, min_score, d[4], d[5], d[6], record_out, d[2], d[3]) &&
              planes.Download();
    for (int k = 0; ok && k < 3; ++k)
        if (nodes[k]) ok = CopyData2DFromDevice(d[4 + k], *nodes[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::CorrelationPassesOk(size_t width, size_t height, float lo, float scale, const CorrelationPass* passes, size_t count,
                                        float min_score, const ValidationOptions& validation)
{
    if (!passes || count < 1 || count > FLOW2D_CORRELATION_MAX_PASSES) {
        std::printf("Error: multi-pass window correlation takes 1 .. %d passes (%zu).\n", FLOW2D_CORRELATION_MAX_PASSES, count);
        return false;
    }
    if (!(std::isfinite(validation.threshold) && validation.threshold > 0.f) ||
        !(std::isfinite(validation.epsilon) && validation.epsilon > 0.f) || validation.min_neighbours < 1 ||
        validation.min_neighbours > 8) {
        std::printf("Error: the validation between passes takes a finite threshold > 0 (%g), a finite epsilon > 0 (%g) and 1 .. 8 "
                    "neighbours at least (%d).\n",
                    validation.threshold, validation.epsilon, validation.min_neighbours);
        return false;
    }
    for (size_t k = 0; k < count; ++k) {
        if (CorrelationArgsOk(width, height, lo, scale, passes[k].radius, passes[k].range, passes[k].spacing, min_score)) continue;
        std::printf("Error: pass %zu of %zu (radius %d : range %d : spacing %d) is refused.\n", k + 1, count, passes[k].radius,
                    passes[k].range, passes[k].spacing);
        return false;
    }
    // an explicit min_pixels has to fit every pass's window (looked at whether or not there is a mask: it needs no device)
    for (size_t k = 0; validation.min_pixels != 0 && k < count; ++k) {
        const int side = 2 * passes[k].radius + 1;
        if (validation.min_pixels >= 1 && validation.min_pixels <= side * side) continue;
        std::printf("Error: a masked window search takes 1 .. (2 radius + 1)^2 pixels at least (%d at radius %d in pass %zu), or 0 for a "
                    "quarter of each pass's window.\n",
                    validation.min_pixels, passes[k].radius, k + 1);
        return false;
    }
    return true;
}

int OpticalFlow2D::CorrelationMinPixels(const ValidationOptions& validation, int radius)
{
    const int side = 2 * radius + 1;
    return validation.min_pixels ? validation.min_pixels : std::max(6, (side * side + 3) / 4);
}

bool OpticalFlow2D::CorrelateMultiPassDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale,
                                             const CorrelationPass* passes, size_t count, float min_score,
                                             const ValidationOptions& validation, DevicePtr dev_predictor_u, DevicePtr dev_predictor_v,
                                             DevicePtr dev_node_u, DevicePtr dev_node_v, DevicePtr dev_node_score,
                                             CorrelationPassReport* reports_out, DevicePtr dev_flow_u, DevicePtr dev_flow_v)
{
    return QueueCorrelationPasses(dev_frame_0, dev_frame_1, lo, scale, passes, count, min_score, validation, dev_predictor_u,
                                  dev_predictor_v, dev_node_u, dev_node_v, dev_node_score, reports_out, dev_flow_u, dev_flow_v, true);
}

bool OpticalFlow2D::QueueCorrelationPasses(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale,
                                           const CorrelationPass* passes, size_t count, float min_score,
                                           const ValidationOptions& validation, DevicePtr dev_predictor_u, DevicePtr dev_predictor_v,
                                           DevicePtr dev_node_u, DevicePtr dev_node_v, DevicePtr dev_node_score,
                                           CorrelationPassReport* reports_out, DevicePtr dev_flow_u, DevicePtr dev_flow_v,
                                           bool synchronise)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!CorrelationPassesOk(W, H, lo, scale, passes, count, min_score, validation)) return false;
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || (dev_flow_u == 0) != (dev_flow_v == 0) ||
        (dev_predictor_u == 0) != (dev_predictor_v == 0) || (dev_node_u == 0) != (dev_node_v == 0))
        return false;
    if (RefuseGroup("multi-pass window correlation")) return false;
    {
        // the caller's written planes pass through the validation and the expansion, which know no frame: checked here
        std::vector<DevicePtr> read = {dev_frame_0, dev_frame_1}, written;
        for (DevicePtr p : {dev_predictor_u, dev_predictor_v, validation.mask})
            if (p) read.push_back(p);
        for (DevicePtr p : {dev_node_u, dev_node_v, dev_node_score, dev_flow_u, dev_flow_v})
            if (p) written.push_back(p);
        if (!WrittenPlanesOk(read.data(), read.size(), written.data(), written.size(), "node, score or flow plane")) return false;
    }
    if (!EnsurePlanes(multipass_planes_, 6)) return false;
    const DevicePtr* own = multipass_planes_.data();
    // per pass: the correlation's record, then the validation's
    const size_t pair = sizeof(flow2d_correlation_pass_record) + sizeof(flow2d_validation_record);
    if (!multipass_scratch_.Ensure(context_, count * pair)) return false;
    const float* predictor[2] = {dev_predictor_u ? AsPlane(dev_predictor_u) : nullptr, dev_predictor_u ? AsPlane(dev_predictor_v) : nullptr};
    bool ok = true;
    for (size_t k = 0; ok && k < count; ++k) {
        const bool last = k + 1 == count, validated = !last || validation.validate_last;
        const CorrelationPass& pass = passes[k];
        auto* record = multipass_scratch_.At<flow2d_correlation_pass_record>(k * pair);
        auto* checked = multipass_scratch_.At<flow2d_validation_record>(k * pair + sizeof(flow2d_correlation_pass_record));
        size_t nw = 0, nh = 0;
        flow2d_correlation_grid(W, H, pass.radius, pass.spacing, &nw, &nh);
        // where the pass's final nodes go: the caller's planes after the last pass, when there are any
        DevicePtr final_u = last && dev_node_u ? dev_node_u : own[validated ? 2 : 0];
        DevicePtr final_v = last && dev_node_v ? dev_node_v : own[validated ? 3 : 1];
        DevicePtr raw_u = validated ? own[0] : final_u, raw_v = validated ? own[1] : final_v;
        // (the node planes are containers: the frames' pitch)
        // With a region of interest both steps are the masked entries, in every pass; the expansion stays as it is: it skips the NaN
        // of a masked node, so the predictor continues the specimen's motion outward.  Without one: the calls there always were.
        if (validation.mask)
            ok = !CheckFlow2DError(flow2d_correlate_masked_2d(context_, AsPlane(dev_frame_0), AsPlane(dev_frame_1), predictor[0],
                                                              predictor[1], W, H, pitch, lo, scale, pass.radius, pass.range, pass.spacing,
                                                              min_score, AsPlane(validation.mask),
                                                              CorrelationMinPixels(validation, pass.radius), AsPlane(raw_u), AsPlane(raw_v),
                                                              last && dev_node_score ? AsPlane(dev_node_score) : nullptr, pitch, record),
                                   "flow2d_correlate_masked_2d");
        else
            ok = !CheckFlow2DError(flow2d_correlate_offset_2d(context_, AsPlane(dev_frame_0), AsPlane(dev_frame_1), predictor[0], predictor[1],
                                                              W, H, pitch, lo, scale, pass.radius, pass.range, pass.spacing, min_score,
                                                              AsPlane(raw_u), AsPlane(raw_v),
                                                              last && dev_node_score ? AsPlane(dev_node_score) : nullptr, pitch, record),
                                   "flow2d_correlate_offset_2d");
        const int mode = !last || validation.replace ? FLOW2D_VALIDATE_REPLACE : FLOW2D_VALIDATE_FLAG;
        if (ok && validated && validation.mask)
            ok = !CheckFlow2DError(flow2d_validate_nodes_masked_2d(context_, AsPlane(raw_u), AsPlane(raw_v), nw, nh, pitch,
                                                                   validation.threshold, validation.epsilon, validation.min_neighbours, mode,
                                                                   AsPlane(validation.mask), W, H, pitch, pass.radius, pass.spacing,
                                                                   AsPlane(final_u), AsPlane(final_v), nullptr, checked),
                                   "flow2d_validate_nodes_masked_2d");
        else if (ok && validated)
            ok = !CheckFlow2DError(flow2d_validate_nodes_2d(context_, AsPlane(raw_u), AsPlane(raw_v), nw, nh, pitch, validation.threshold,
                                                            validation.epsilon, validation.min_neighbours, mode, AsPlane(final_u),
                                                            AsPlane(final_v), nullptr, checked),
                                   "flow2d_validate_nodes_2d");
        if (ok && !last) {
            ok = !CheckFlow2DError(flow2d_expand_nodes_2d(context_, AsPlane(final_u), AsPlane(final_v), nw, nh, pitch, pass.radius,
                                                          pass.spacing, AsPlane(own[4]), AsPlane(own[5]), W, H, pitch),
                                   "flow2d_expand_nodes_2d");
            predictor[0] = AsPlane(own[4]);
            predictor[1] = AsPlane(own[5]);
        } else if (ok && dev_flow_u) {
            ok = !CheckFlow2DError(flow2d_expand_nodes_2d(context_, AsPlane(final_u), AsPlane(final_v), nw, nh, pitch, pass.radius,
                                                          pass.spacing, AsPlane(dev_flow_u), AsPlane(dev_flow_v), W, H, pitch),
                                   "flow2d_expand_nodes_2d");
        }
        if (ok && reports_out) {
            CorrelationPassReport& report = reports_out[k];
            report = CorrelationPassReport{};
            report.nw = nw;
            report.nh = nh;
            ok = ReadRecord(&report.correlation, record, sizeof(report.correlation)) &&
                 (!validated || ReadRecord(&report.validation, checked, sizeof(report.validation)));
        }
    }
    if (!synchronise) return ok;
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

namespace {
// The node images of the host forms: eight -- u, v, ux, uy, vx, vy, score, state --, and at order 2 the six curvatures behind them.
int NodeImages(const OpticalFlow2D::SubsetOptions& subset) { return subset.order == 2 ? 14 : 8; }
// Whether the curvature images (order 2) come all or none.
bool CurvatureImagesOk(Data2D* const* nodes, int count)
{
    for (int k = 9; k < count; ++k)
        if ((nodes[k] != nullptr) != (nodes[8] != nullptr)) return false;
    return true;
}
OpticalFlow2D::SubsetPlanes NodePlanes(const DevicePtr* d, int count)
{
    OpticalFlow2D::SubsetPlanes out = {d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]};
    if (count == 14) {
        out.uxx = d[8];
        out.uxy = d[9];
        out.uyy = d[10];
        out.vxx = d[11];
        out.vxy = d[12];
        out.vyy = d[13];
    }
    return out;
}
}  // namespace

int OpticalFlow2D::SubsetMinPixels(const SubsetOptions& subset)
{
    const int side = 2 * subset.radius + 1;
    return subset.min_pixels ? subset.min_pixels : std::max(FLOW2D_SUBSET_MIN_PIXELS, (side * side + 3) / 4);
}

bool OpticalFlow2D::SubsetOptionsOk(const SubsetOptions& subset)
{
    if (subset.mask && subset.order == 2) {
        std::printf("Error: a subset mask goes with the first-order refinement only (order %d): flow2d_subset_refine2_2d takes no mask.\n",
                    subset.order);
        return false;
    }
    if (subset.mask_search && !subset.mask) {
        std::printf("Error: a masked window search in front of the subset refinement needs the subset mask.\n");
        return false;
    }
    if (subset.min_pixels != 0 && (subset.min_pixels < FLOW2D_SUBSET_MIN_PIXELS ||
                                   (subset.radius >= 1 && subset.radius <= FLOW2D_SUBSET_MAX_RADIUS &&
                                    subset.min_pixels > (2 * subset.radius + 1) * (2 * subset.radius + 1)))) {
        std::printf("Error: a masked subset refinement takes %d .. (2 radius + 1)^2 pixels at least (%d at radius %d), or 0 for a quarter "
                    "of the subset.\n",
                    FLOW2D_SUBSET_MIN_PIXELS, subset.min_pixels, subset.radius);
        return false;
    }
    if (subset.interpolation != SubsetOptions::CatmullRom && subset.interpolation != SubsetOptions::BSpline) {
        std::printf("Error: subset refinement samples frame 1 with Catmull-Rom weights (%d) or a cubic B-spline (%d), not %d.\n",
                    SubsetOptions::CatmullRom, SubsetOptions::BSpline, subset.interpolation);
        return false;
    }
    if (subset.radius >= 1 && subset.radius <= FLOW2D_SUBSET_MAX_RADIUS && subset.iterations >= 1 &&
        subset.iterations <= FLOW2D_SUBSET_MAX_ITERATIONS && std::isfinite(subset.epsilon) && subset.epsilon >= 0.f &&
        std::isfinite(subset.max_shift) && subset.max_shift > 0.f && std::isfinite(subset.max_gradient) && subset.max_gradient > 0.f &&
        (subset.order == 1 || (subset.order == 2 && subset.radius >= FLOW2D_SUBSET2_MIN_RADIUS)) && std::isfinite(subset.max_curvature) &&
        subset.max_curvature > 0.f)
        return true;
    std::printf("Error: subset refinement takes a radius of 1 .. %d (%d), 1 .. %d iterations (%d), a finite epsilon >= 0 (%g), a finite "
                "largest shift > 0 (%g) and a finite largest gradient > 0 (%g); an order of 1 or 2 (%d), at order 2 a radius from %d, and a "
                "finite largest curvature > 0 (%g).\n",
                FLOW2D_SUBSET_MAX_RADIUS, subset.radius, FLOW2D_SUBSET_MAX_ITERATIONS, subset.iterations, subset.epsilon, subset.max_shift,
                subset.max_gradient, subset.order, FLOW2D_SUBSET2_MIN_RADIUS, subset.max_curvature);
    return false;
}

bool OpticalFlow2D::QueueRefineNodes(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_node_u0, DevicePtr dev_node_v0,
                                     int grid_radius, int spacing, const SubsetOptions& subset, const SubsetPlanes& out,
                                     flow2d_subset_record* record_out, DevicePtr* refined, const DevicePtr* start_gradients)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!SubsetOptionsOk(subset)) return false;
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(W, H, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) {
        std::printf("Error: a %zu x %zu frame holds no node grid of radius %d and spacing %d.\n", W, H, grid_radius, spacing);
        return false;
    }
    const bool gradients = out.ux != 0, curvatures = out.uxx != 0;
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || !dev_node_u0 || !dev_node_v0 || (out.u == 0) != (out.v == 0) ||
        (out.uy != 0) != gradients || (out.vx != 0) != gradients || (out.vy != 0) != gradients || (out.uxy != 0) != curvatures ||
        (out.uyy != 0) != curvatures || (out.vxx != 0) != curvatures || (out.vxy != 0) != curvatures || (out.vyy != 0) != curvatures)
        return false;
    if (curvatures && subset.order != 2) {
        std::printf("Error: '%s': curvature planes are written by the second-order refinement only.\n", GetName());
        return false;
    }
    if (RefuseGroup("subset refinement")) return false;
    if (!EnsurePlanes(subset_planes_, 4)) return false;
    const DevicePtr u = out.u ? out.u : subset_planes_[2], v = out.v ? out.v : subset_planes_[3];
    if (record_out && !subset_scratch_.Ensure(context_, sizeof(flow2d_subset_record))) return false;
    flow2d_subset_record* record = record_out ? subset_scratch_.At<flow2d_subset_record>() : nullptr;
    auto plane = [](DevicePtr p) { return p ? AsPlane(p) : nullptr; };
    // (the node planes are containers: the frames' pitch; the entry refuses planes that meet)
    bool ok;
    const bool spline = subset.interpolation == SubsetOptions::BSpline;
    if (spline) {
        // frame 1's coefficients, on the same stream in front of the refinement that samples them
        if (!EnsurePlanes(spline_plane_, 1) ||
            CheckFlow2DError(flow2d_bspline_prefilter_2d(context_, AsPlane(dev_frame_1), AsPlane(spline_plane_[0]), W, H, pitch),
                             "flow2d_bspline_prefilter_2d"))
            return false;
    }
    if (subset.order == 2) {
        // the start: the gradients where the caller has them, no curvatures (0)
        const float* start[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int k = 0; start_gradients && k < 4; ++k) start[k] = plane(start_gradients[k]);
        float* const out_gradients[4] = {plane(out.ux), plane(out.uy), plane(out.vx), plane(out.vy)};
        float* const out_curvatures[6] = {plane(out.uxx), plane(out.uxy), plane(out.uyy), plane(out.vxx), plane(out.vxy), plane(out.vyy)};
        if (spline)
            ok = !CheckFlow2DError(flow2d_subset_refine2_spline_2d(context_, AsPlane(dev_frame_0), AsPlane(spline_plane_[0]), W, H, pitch,
                                                                   AsPlane(dev_node_u0), AsPlane(dev_node_v0), start_gradients ? start : nullptr,
                                                                   nullptr, nw, nh, pitch, grid_radius, spacing, subset.radius,
                                                                   subset.iterations, subset.epsilon, subset.max_shift, subset.max_gradient,
                                                                   subset.max_curvature, AsPlane(u), AsPlane(v), out_gradients, out_curvatures,
                                                                   plane(out.score), plane(out.state), record),
                                   "flow2d_subset_refine2_spline_2d");
        else
            ok = !CheckFlow2DError(flow2d_subset_refine2_2d(context_, AsPlane(dev_frame_0), AsPlane(dev_frame_1), W, H, pitch,
                                                            AsPlane(dev_node_u0), AsPlane(dev_node_v0), start_gradients ? start : nullptr,
                                                            nullptr, nw, nh, pitch, grid_radius, spacing, subset.radius, subset.iterations,
                                                            subset.epsilon, subset.max_shift, subset.max_gradient, subset.max_curvature,
                                                            AsPlane(u), AsPlane(v), out_gradients, out_curvatures, plane(out.score),
                                                            plane(out.state), record),
                                   "flow2d_subset_refine2_2d");
    } else if (spline) {
        // (one entry for every first-order call: mask and start gradients may both be absent)
        const DevicePtr none[4] = {0, 0, 0, 0};
        const DevicePtr* g = start_gradients ? start_gradients : none;
        ok = !CheckFlow2DError(flow2d_subset_refine_spline_2d(context_, AsPlane(dev_frame_0), AsPlane(spline_plane_[0]), W, H, pitch,
                                                              AsPlane(dev_node_u0), AsPlane(dev_node_v0), plane(g[0]), plane(g[1]), plane(g[2]),
                                                              plane(g[3]), nw, nh, pitch, grid_radius, spacing, subset.radius,
                                                              subset.iterations, subset.epsilon, subset.max_shift, subset.max_gradient,
                                                              plane(subset.mask), SubsetMinPixels(subset), AsPlane(u), AsPlane(v),
                                                              plane(out.ux), plane(out.uy), plane(out.vx), plane(out.vy), plane(out.score),
                                                              plane(out.state), record),
                               "flow2d_subset_refine_spline_2d");
    } else if (subset.mask) {
        // (without a start the entry takes the zero gradients of flow2d_subset_refine_2d)
        const DevicePtr none[4] = {0, 0, 0, 0};
        const DevicePtr* g = start_gradients ? start_gradients : none;
        ok = !CheckFlow2DError(flow2d_subset_refine_masked_2d(context_, AsPlane(dev_frame_0), AsPlane(dev_frame_1), W, H, pitch,
                                                              AsPlane(dev_node_u0), AsPlane(dev_node_v0), plane(g[0]), plane(g[1]), plane(g[2]),
                                                              plane(g[3]), nw, nh, pitch, grid_radius, spacing, subset.radius,
                                                              subset.iterations, subset.epsilon, subset.max_shift, subset.max_gradient,
                                                              AsPlane(subset.mask), SubsetMinPixels(subset), AsPlane(u), AsPlane(v),
                                                              plane(out.ux), plane(out.uy), plane(out.vx), plane(out.vy), plane(out.score),
                                                              plane(out.state), record),
                               "flow2d_subset_refine_masked_2d");
    } else if (start_gradients)
        ok = !CheckFlow2DError(flow2d_subset_refine_from_2d(context_, AsPlane(dev_frame_0), AsPlane(dev_frame_1), W, H, pitch,
                                                            AsPlane(dev_node_u0), AsPlane(dev_node_v0), plane(start_gradients[0]),
                                                            plane(start_gradients[1]), plane(start_gradients[2]),
                                                            plane(start_gradients[3]), nw, nh, pitch, grid_radius, spacing, subset.radius,
                                                            subset.iterations, subset.epsilon, subset.max_shift, subset.max_gradient,
                                                            AsPlane(u), AsPlane(v), plane(out.ux), plane(out.uy), plane(out.vx),
                                                            plane(out.vy), plane(out.score), plane(out.state), record),
                               "flow2d_subset_refine_from_2d");
    else
        ok = !CheckFlow2DError(flow2d_subset_refine_2d(context_, AsPlane(dev_frame_0), AsPlane(dev_frame_1), W, H, pitch,
                                                       AsPlane(dev_node_u0), AsPlane(dev_node_v0), nw, nh, pitch, grid_radius, spacing,
                                                       subset.radius, subset.iterations, subset.epsilon, subset.max_shift,
                                                       subset.max_gradient, AsPlane(u), AsPlane(v), plane(out.ux), plane(out.uy),
                                                       plane(out.vx), plane(out.vy), plane(out.score), plane(out.state), record),
                               "flow2d_subset_refine_2d");
    ok = ok && (!record_out || ReadRecord(record_out, record, sizeof(*record_out)));
    if (refined) {
        refined[0] = u;
        refined[1] = v;
    }
    return ok;
}

bool OpticalFlow2D::RefineNodesDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_node_u0, DevicePtr dev_node_v0,
                                      int grid_radius, int spacing, const SubsetOptions& subset, const SubsetPlanes& out,
                                      flow2d_subset_record* record_out)
{
    const bool ok = QueueRefineNodes(dev_frame_0, dev_frame_1, dev_node_u0, dev_node_v0, grid_radius, spacing, subset, out, record_out, nullptr);
    if (!ok || !record_out) return ok;
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize");
}

bool OpticalFlow2D::CorrelateSubsetDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, const CorrelationPass* passes,
                                          size_t count, float min_score, const ValidationOptions& validation, const SubsetOptions& subset,
                                          DevicePtr dev_predictor_u, DevicePtr dev_predictor_v, const SubsetPlanes& out,
                                          CorrelationPassReport* reports_out, flow2d_subset_record* record_out, DevicePtr dev_flow_u,
                                          DevicePtr dev_flow_v)
{
    return QueueCorrelateSubset(dev_frame_0, dev_frame_1, lo, scale, passes, count, min_score, validation, subset, dev_predictor_u,
                                dev_predictor_v, out, reports_out, record_out, dev_flow_u, dev_flow_v, true);
}

bool OpticalFlow2D::QueueCorrelateSubset(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, const CorrelationPass* passes,
                                         size_t count, float min_score, const ValidationOptions& validation, const SubsetOptions& subset,
                                         DevicePtr dev_predictor_u, DevicePtr dev_predictor_v, const SubsetPlanes& out,
                                         CorrelationPassReport* reports_out, flow2d_subset_record* record_out, DevicePtr dev_flow_u,
                                         DevicePtr dev_flow_v, bool synchronise)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!CorrelationPassesOk(W, H, lo, scale, passes, count, min_score, validation) || !SubsetOptionsOk(subset)) return false;
    const bool gradients = out.ux != 0;
    if (!IsInitialized() || (dev_flow_u == 0) != (dev_flow_v == 0) || (out.u == 0) != (out.v == 0) || (out.uy != 0) != gradients ||
        (out.vx != 0) != gradients || (out.vy != 0) != gradients)
        return false;
    if (RefuseGroup("subset refinement")) return false;
    if (!EnsurePlanes(subset_planes_, 4)) return false;
    ValidationOptions every_node = validation;  // the last pass fills what it did not find: every node gets a start
    every_node.validate_last = true;
    every_node.replace = true;
    if (subset.mask_search) every_node.mask = subset.mask;  // (SubsetOptionsOk: there is one)
    const CorrelationPass& fine = passes[count - 1];
    DevicePtr refined[2] = {0, 0};
    bool ok = QueueCorrelationPasses(dev_frame_0, dev_frame_1, lo, scale, passes, count, min_score, every_node, dev_predictor_u,
                                     dev_predictor_v, subset_planes_[0], subset_planes_[1], 0, reports_out, 0, 0, false) &&
              QueueRefineNodes(dev_frame_0, dev_frame_1, subset_planes_[0], subset_planes_[1], fine.radius, fine.spacing, subset, out,
                               record_out, refined);
    if (ok && dev_flow_u) {
        size_t nw = 0, nh = 0;
        flow2d_correlation_grid(W, H, fine.radius, fine.spacing, &nw, &nh);
        ok = !CheckFlow2DError(flow2d_expand_nodes_2d(context_, AsPlane(refined[0]), AsPlane(refined[1]), nw, nh, pitch, fine.radius,
                                                      fine.spacing, AsPlane(dev_flow_u), AsPlane(dev_flow_v), W, H, pitch),
                               "flow2d_expand_nodes_2d");
    }
    if (!synchronise) return ok;
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::CorrelateSubset(Data2D& frame_0, Data2D& frame_1, const CorrelationPass* passes, size_t count, float min_score,
                                    const ValidationOptions& validation, const SubsetOptions& subset, Data2D* const* nodes,
                                    CorrelationPassReport* reports_out, flow2d_subset_record* record_out, Data2D* flow_u, Data2D* flow_v,
                                    Data2D* predictor_u, Data2D* predictor_v, Data2D* mask)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !nodes || !nodes[0] || !nodes[1] || (flow_u == nullptr) != (flow_v == nullptr) ||
        (predictor_u == nullptr) != (predictor_v == nullptr))
        return;
    const bool gradients = nodes[2] != nullptr;
    if ((nodes[3] != nullptr) != gradients || (nodes[4] != nullptr) != gradients || (nodes[5] != nullptr) != gradients) return;
    const int images = NodeImages(subset);
    if (!CurvatureImagesOk(nodes, images)) return;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In).Add(flow_u, CallPlanes::Out).Add(flow_v, CallPlanes::Out);
    // the node planes: containers with no image of their size behind them, downloaded below
    for (int k = 0; k < images; ++k) planes.Add(nullptr, CallPlanes::Out, nodes[k] != nullptr);
    if (predictor_u) planes.Add(predictor_u, CallPlanes::In).Add(predictor_v, CallPlanes::In);
    const int mask_at = 4 + images + (predictor_u ? 2 : 0);  // the mask, uploaded once, behind everything else
    if (mask) planes.Add(mask, CallPlanes::In);
    if (!planes.SizesMatch()) return;
    float lo = 0.f, scale = 1.f;
    CorrelationRange(frame_0, frame_1, lo, scale);
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    SubsetOptions masked = subset;
    masked.mask = mask ? 1 : 0;  // (for the check; the plane's address below)
    if (!CorrelationPassesOk(W, H, lo, scale, passes, count, min_score, validation) || !SubsetOptionsOk(masked)) return;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(W, H, passes[count - 1].radius, passes[count - 1].spacing, &nw, &nh);
    for (int k = 0; k < images; ++k)
        if (nodes[k] && (nodes[k]->Width() != nw || nodes[k]->Height() != nh)) {
            std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
            return;
        }
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    const SubsetPlanes out = NodePlanes(d + 4, images);
    masked.mask = mask ? d[mask_at] : 0;
    bool ok = planes.Upload() &&
              CorrelateSubsetDevice(d[0], d[1], lo, scale, passes, count, min_score, validation, masked, predictor_u ? d[4 + images] : 0,
                                    predictor_u ? d[5 + images] : 0, out, reports_out, record_out, d[2], d[3]) &&
              planes.Download();
    for (int k = 0; ok && k < images; ++k)
        if (nodes[k]) ok = CopyData2DFromDevice(d[4 + k], *nodes[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::RefineNodesFromDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, const SubsetPlanes& start, int grid_radius,
                                          int spacing, const SubsetOptions& subset, const SubsetPlanes& out,
                                          flow2d_subset_record* record_out)
{
    if (!start.u || !start.v || !start.ux || !start.uy || !start.vx || !start.vy) return false;
    const DevicePtr gradients[4] = {start.ux, start.uy, start.vx, start.vy};
    const bool ok = QueueRefineNodes(dev_frame_0, dev_frame_1, start.u, start.v, grid_radius, spacing, subset, out, record_out, nullptr, gradients);
    if (!ok || !record_out) return ok;
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize");
}

bool OpticalFlow2D::SequenceOptionsOk(const SequenceOptions& sequence)
{
    if (sequence.reference_every < 0) {
        std::printf("Error: a subset sequence takes a new reference frame every N >= 1 steps, or 0 for never (%d).\n",
                    sequence.reference_every);
        return false;
    }
    if (sequence.fill >= 1 && sequence.fill <= kSequenceMaxFill && (sequence.min_state == 0 || sequence.min_state == 1) &&
        sequence.min_neighbours >= 1 && sequence.min_neighbours <= 8 && std::isfinite(sequence.max_shift) && sequence.max_shift > 0.f)
        return true;
    std::printf("Error: a subset sequence takes 1 .. %d prediction passes (%d), a least state of 0 or 1 (%d), 1 .. 8 neighbours at least "
                "(%d) and a finite largest shift > 0 (%g).\n",
                kSequenceMaxFill, sequence.fill, sequence.min_state, sequence.min_neighbours, sequence.max_shift);
    return false;
}

bool OpticalFlow2D::QueueSequenceStep(DevicePtr dev_frame_0, DevicePtr dev_frame_k, const SubsetPlanes& last, int grid_radius, int spacing,
                                      const SubsetOptions& subset, const SequenceOptions& sequence, const SubsetPlanes& out,
                                      SequenceStepReport* report_out, size_t scratch_offset, DevicePtr dev_flow_u, DevicePtr dev_flow_v)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(W, H, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) {
        std::printf("Error: a %zu x %zu frame holds no node grid of radius %d and spacing %d.\n", W, H, grid_radius, spacing);
        return false;
    }
    // the prediction's passes: from the last step's planes into set 0, from there into set 1, and back
    const float* in[7] = {AsPlane(last.u),  AsPlane(last.v),  AsPlane(last.ux),   AsPlane(last.uy),
                          AsPlane(last.vx), AsPlane(last.vy), AsPlane(last.state)};
    const DevicePtr* set = nullptr;
    bool ok = true;
    for (int pass = 0; ok && pass < sequence.fill; ++pass) {
        set = sequence_planes_.data() + 7 * (pass & 1);
        auto* record = sequence_scratch_.At<flow2d_predict_record>(scratch_offset + sizeof(flow2d_subset_record) +
                                                                    pass * sizeof(flow2d_predict_record));
        ok = !CheckFlow2DError(flow2d_predict_nodes_2d(context_, in[0], in[1], in[2], in[3], in[4], in[5], in[6], nw, nh, pitch, spacing,
                                                       sequence.min_state, sequence.min_neighbours, AsPlane(set[0]), AsPlane(set[1]),
                                                       AsPlane(set[2]), AsPlane(set[3]), AsPlane(set[4]), AsPlane(set[5]), AsPlane(set[6]),
                                                       report_out ? record : nullptr),
                               "flow2d_predict_nodes_2d");
        if (ok && report_out) ok = ReadRecord(&report_out->prediction[pass], record, sizeof(*record));
        for (int c = 0; c < 7; ++c) in[c] = AsPlane(set[c]);
    }
    if (!ok) return false;
    DevicePtr refined[2] = {0, 0};
    ok = QueueRefineNodes(dev_frame_0, dev_frame_k, set[0], set[1], grid_radius, spacing, subset, out, report_out ? &report_out->subset : nullptr,
                          refined, set + 2);
    if (ok && dev_flow_u)
        ok = !CheckFlow2DError(flow2d_expand_nodes_2d(context_, AsPlane(refined[0]), AsPlane(refined[1]), nw, nh, pitch, grid_radius, spacing,
                                                      AsPlane(dev_flow_u), AsPlane(dev_flow_v), W, H, pitch),
                               "flow2d_expand_nodes_2d");
    return ok;
}

bool OpticalFlow2D::ContinueSubsetSequenceDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_k, const SubsetPlanes& previous, int grid_radius,
                                                 int spacing, const SubsetOptions& subset, const SequenceOptions& sequence,
                                                 const SubsetPlanes& out, SequenceStepReport* report_out, DevicePtr dev_flow_u,
                                                 DevicePtr dev_flow_v)
{
    SubsetOptions later = subset;
    later.max_shift = sequence.max_shift;
    if (!SubsetOptionsOk(later) || !SequenceOptionsOk(sequence)) return false;
    const bool gradients = out.ux != 0;
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_k || !previous.u || !previous.v || !previous.ux || !previous.uy || !previous.vx ||
        !previous.vy || !previous.state || (dev_flow_u == 0) != (dev_flow_v == 0) || (out.u == 0) != (out.v == 0) ||
        (out.uy != 0) != gradients || (out.vx != 0) != gradients || (out.vy != 0) != gradients)
        return false;
    if (RefuseGroup("a subset sequence")) return false;
    {
        const DevicePtr read[] = {dev_frame_0, dev_frame_k, previous.u, previous.v, previous.ux, previous.uy, previous.vx, previous.vy, previous.state};
        std::vector<DevicePtr> written;
        for (DevicePtr p : {out.u, out.v, out.ux, out.uy, out.vx, out.vy, out.score, out.state, dev_flow_u, dev_flow_v, out.uxx, out.uxy,
                            out.uyy, out.vxx, out.vxy, out.vyy})
            if (p) written.push_back(p);
        if (!WrittenPlanesOk(read, 9, written.data(), written.size(), "node or flow plane")) return false;
    }
    if (!EnsurePlanes(sequence_planes_, 14)) return false;
    if (!sequence_scratch_.Ensure(context_, sizeof(flow2d_subset_record) + kSequenceMaxFill * sizeof(flow2d_predict_record))) return false;
    if (report_out) *report_out = SequenceStepReport{};
    const bool ok = QueueSequenceStep(dev_frame_0, dev_frame_k, previous, grid_radius, spacing, later, sequence, out, report_out, 0, dev_flow_u,
                                      dev_flow_v);
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::ContinueSubsetSequence(Data2D& frame_0, Data2D& frame_k, Data2D* const* previous, int grid_radius, int spacing,
                                           const SubsetOptions& subset, const SequenceOptions& sequence, Data2D* const* nodes,
                                           SequenceStepReport* report_out, Data2D* flow_u, Data2D* flow_v, Data2D* mask)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !previous || !nodes || !nodes[0] || !nodes[1] || (flow_u == nullptr) != (flow_v == nullptr)) return;
    for (int k = 0; k < 7; ++k)
        if (!previous[k]) return;
    const bool gradients = nodes[2] != nullptr;
    if ((nodes[3] != nullptr) != gradients || (nodes[4] != nullptr) != gradients || (nodes[5] != nullptr) != gradients) return;
    const int images = NodeImages(subset);
    if (!CurvatureImagesOk(nodes, images)) return;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(W, H, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) {
        std::printf("Error: a %zu x %zu frame holds no node grid of radius %d and spacing %d.\n", W, H, grid_radius, spacing);
        return;
    }
    for (int k = 0; k < 7 + images; ++k) {
        Data2D* image = k < 7 ? previous[k] : nodes[k - 7];
        if (image && (image->Width() != nw || image->Height() != nh)) {
            std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
            return;
        }
    }
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_k, CallPlanes::In).Add(flow_u, CallPlanes::Out).Add(flow_v, CallPlanes::Out);
    // the node planes, read and written: containers with no image of their size behind them, uploaded and downloaded here
    for (int k = 0; k < 7; ++k) planes.Add(nullptr, CallPlanes::Out, true);
    for (int k = 0; k < images; ++k) planes.Add(nullptr, CallPlanes::Out, nodes[k] != nullptr);
    if (mask) planes.Add(mask, CallPlanes::In);  // uploaded once, behind everything else
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    bool ok = planes.Upload();
    for (int k = 0; ok && k < 7; ++k) ok = CopyData2DtoDevice(*previous[k], d[4 + k], H, dev_container_size_.pitch);
    const SubsetPlanes last = {d[4], d[5], d[6], d[7], d[8], d[9], 0, d[10]};
    const SubsetPlanes out = NodePlanes(d + 11, images);
    SubsetOptions masked = subset;
    masked.mask = mask ? d[11 + images] : 0;
    ok = ok && ContinueSubsetSequenceDevice(d[0], d[1], last, grid_radius, spacing, masked, sequence, out, report_out, d[2], d[3]) &&
         planes.Download();
    for (int k = 0; ok && k < images; ++k)
        if (nodes[k]) ok = CopyData2DFromDevice(d[11 + k], *nodes[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::StrainOptionsOk(const StrainOptions& strain)
{
    const int k = strain.order == 2 ? 6 : 3, side = 2 * strain.window + 1;
    if (strain.window >= 0 && strain.window <= FLOW2D_NODE_STRAIN_MAX_WINDOW && (strain.min_state == 0 || strain.min_state == 1) &&
        (strain.measure == FLOW2D_STRAIN_SMALL || strain.measure == FLOW2D_STRAIN_GREEN_LAGRANGE) &&
        (strain.window == 0 ||
         ((strain.order == 1 || strain.order == 2) && (strain.min_nodes == 0 || (strain.min_nodes >= k && strain.min_nodes <= side * side))))) {
        if (strain.weighted) {
            if (strain.robust_sigma != 0.f) {
                std::printf("Error: weighted node strain takes its threshold in sigmas (%g) and a robust scale is in pixels (%g): the two "
                            "exclude each other.\n",
                            static_cast<double>(strain.weight_threshold), static_cast<double>(strain.robust_sigma));
                return false;
            }
            if (strain.window >= 1 && std::isfinite(strain.sigma_floor) && strain.sigma_floor >= 0.f &&
                std::isfinite(strain.weight_threshold) && strain.weight_threshold >= 0.f &&
                (strain.weight_threshold == 0.f ||
                 (strain.robust_iterations >= 0 && strain.robust_iterations <= FLOW2D_NODE_STRAIN_MAX_ITERATIONS)))
                return true;
            std::printf("Error: weighted node strain takes a window of 1 or more nodes (%d), a floor (%g) and a threshold (%g) that are "
                        "finite and not negative and, with a threshold, 0 .. %d reweighted passes (%d).\n",
                        strain.window, static_cast<double>(strain.sigma_floor), static_cast<double>(strain.weight_threshold),
                        FLOW2D_NODE_STRAIN_MAX_ITERATIONS, strain.robust_iterations);
            return false;
        }
        // robust_sigma 0 is the plain fit; anything else has to be a scale the robust entry takes, with a window to reweight
        if (strain.robust_sigma == 0.f) return true;
        if (std::isfinite(strain.robust_sigma) && strain.robust_sigma > 0.f && strain.window >= 1 && strain.robust_iterations >= 0 &&
            strain.robust_iterations <= FLOW2D_NODE_STRAIN_MAX_ITERATIONS)
            return true;
        std::printf("Error: robust node strain takes a scale that is finite and positive (%g), a window of 1 or more nodes (%d) and "
                    "0 .. %d reweighted passes (%d).\n",
                    static_cast<double>(strain.robust_sigma), strain.window, FLOW2D_NODE_STRAIN_MAX_ITERATIONS, strain.robust_iterations);
        return false;
    }
    std::printf("Error: node strain takes a window of 0 .. %d nodes (%d), with a window an order of 1 or 2 (%d) and a least node count "
                "of 0 or between the fit's coefficients and the window's nodes (%d), a least state of 0 or 1 (%d) and a measure of 0 or "
                "1 (%d).\n",
                FLOW2D_NODE_STRAIN_MAX_WINDOW, strain.window, strain.order, strain.min_nodes, strain.min_state, strain.measure);
    return false;
}

bool OpticalFlow2D::NodeStrainDevice(const SubsetPlanes* steps, size_t step_count, size_t nw, size_t nh, int spacing,
                                     const StrainOptions& strain, const DevicePtr* out_planes, flow2d_deformation_stats* stats_out,
                                     const DevicePtr* diagnostics)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!StrainOptionsOk(strain)) return false;
    if (strain.weighted) {
        std::printf("Error: '%s': weighted node strain needs the nodes' sigma planes: the form that takes them.\n", GetName());
        return false;
    }
    const bool robust = strain.robust_sigma != 0.f;
    if (diagnostics && !robust) {
        std::printf("Error: '%s': the diagnostic planes of node strain go with a robust scale.\n", GetName());
        return false;
    }
    if (!IsInitialized() || !steps || step_count == 0 || (!out_planes && !stats_out && !diagnostics)) return false;
    if (nw == 0 || nh == 0 || nw > W || nh > H) {
        std::printf("Error: '%s': a %zu x %zu node grid does not lie in planes of %zu x %zu.\n", GetName(), nw, nh, W, H);
        return false;
    }
    if (RefuseGroup("node strain")) return false;
    for (size_t k = 0; k < step_count; ++k) {
        const SubsetPlanes& q = steps[k];
        const bool gradients = q.ux != 0;
        if (!q.u || !q.v || (q.uy != 0) != gradients || (q.vx != 0) != gradients || (q.vy != 0) != gradients ||
            (strain.window == 0 && !gradients)) {
            std::printf("Error: '%s': step %zu of node strain needs u and v, the four gradients all or none, and all with window 0.\n",
                        GetName(), k + 1);
            return false;
        }
    }
    const int min_nodes = strain.window > 0 && strain.min_nodes == 0 ? (strain.order == 2 ? 6 : 3) + 1 : strain.min_nodes;
    const size_t workspace_bytes =
        !stats_out ? 0 : robust ? flow2d_node_strain_robust_workspace_bytes(nw, nh, 1) : flow2d_node_strain_workspace_bytes(nw, nh, 1);
    const size_t per_step = sizeof(flow2d_deformation_stats) + workspace_bytes;
    if (stats_out && !strain_scratch_.Ensure(context_, step_count * per_step)) return false;
    auto plane = [](DevicePtr p) { return p ? AsPlane(p) : nullptr; };
    bool ok = true;
    for (size_t k = 0; ok && k < step_count; ++k) {
        const SubsetPlanes& q = steps[k];
        flow2d_deformation_planes out = {};
        if (out_planes) {
            const DevicePtr* d = out_planes + 9 * k;
            out = {plane(d[0]), plane(d[1]), plane(d[2]), plane(d[3]), plane(d[4]), plane(d[5]), plane(d[6]), plane(d[7]), plane(d[8])};
        }
        auto* record = stats_out ? strain_scratch_.At<flow2d_deformation_stats>(k * per_step) : nullptr;
        void* workspace = stats_out ? strain_scratch_.At<>(k * per_step + sizeof(flow2d_deformation_stats)) : nullptr;
        // (the node planes are containers: the frames' pitch; the entry refuses planes that meet)
        if (robust) {
            flow2d_node_strain_diagnostics diag = {};
            if (diagnostics) diag = {plane(diagnostics[3 * k]), plane(diagnostics[3 * k + 1]), plane(diagnostics[3 * k + 2])};
            ok = !CheckFlow2DError(flow2d_node_strain_robust_2d(context_, AsPlane(q.u), AsPlane(q.v), plane(q.state), nw, nh, pitch, spacing,
                                                                strain.window, strain.order, min_nodes, strain.min_state, strain.measure,
                                                                strain.robust_sigma, strain.robust_iterations, &out, &diag, record,
                                                                workspace, workspace_bytes),
                                   "flow2d_node_strain_robust_2d");
            if (ok && stats_out) ok = ReadRecord(stats_out + k, record, sizeof(*record));
            continue;
        }
        ok = !CheckFlow2DError(flow2d_node_strain_2d(context_, AsPlane(q.u), AsPlane(q.v), plane(q.state), plane(q.ux), plane(q.uy),
                                                     plane(q.vx), plane(q.vy), nw, nh, pitch, spacing, strain.window, strain.order,
                                                     min_nodes, strain.min_state, strain.measure, &out, record, workspace, workspace_bytes),
                               "flow2d_node_strain_2d");
        if (ok && stats_out) ok = ReadRecord(stats_out + k, record, sizeof(*record));
    }
    if (!stats_out) return ok;
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::NodeStrain(Data2D* const* nodes, size_t step_count, int spacing, const StrainOptions& strain, Data2D* const* planes,
                               flow2d_deformation_stats* stats_out, Data2D* const* diagnostics)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !nodes || step_count == 0 || !nodes[0] || (!planes && !stats_out && !diagnostics) || !StrainOptionsOk(strain))
        return;
    const size_t nw = nodes[0]->Width(), nh = nodes[0]->Height(), H = dev_container_size_.height;
    if (nw == 0 || nh == 0 || nw > dev_container_size_.width || nh > H) {
        std::printf("Error: '%s': a %zu x %zu node grid does not lie in planes of %zu x %zu.\n", GetName(), nw, nh,
                    dev_container_size_.width, H);
        return;
    }
    for (size_t k = 0; k < step_count; ++k) {
        if (!nodes[7 * k] || !nodes[7 * k + 1]) return;
        for (int c = 0; c < 19; ++c) {
            Data2D* image = c < 7    ? nodes[7 * k + c]
                            : c < 16 ? (planes ? planes[9 * k + c - 7] : nullptr)
                                     : (diagnostics ? diagnostics[3 * k + c - 16] : nullptr);
            if (image && (image->Width() != nw || image->Height() != nh)) {
                std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
                return;
            }
        }
    }
    // the node planes, read and written: containers with no image of their size behind them, uploaded and downloaded here
    CallPlanes call_planes(context_, dev_container_size_, GetName(), "node");
    for (size_t k = 0; k < step_count; ++k) {
        for (int c = 0; c < 7; ++c) call_planes.Add(nullptr, CallPlanes::Out, nodes[7 * k + c] != nullptr);
        for (int c = 0; c < 9; ++c) call_planes.Add(nullptr, CallPlanes::Out, planes && planes[9 * k + c] != nullptr);
    }
    // (the diagnostic planes lie behind every step's sixteen, so that those keep their places)
    for (size_t k = 0; diagnostics && k < 3 * step_count; ++k) call_planes.Add(nullptr, CallPlanes::Out, diagnostics[k] != nullptr);
    HostCall call(context_, last_total_ms_, call_planes.Allocate());
    const DevicePtr* d = call_planes.data();
    bool ok = call_planes.Upload();
    std::vector<SubsetPlanes> steps(step_count);
    std::vector<DevicePtr> out(9 * step_count, 0);
    for (size_t k = 0; k < step_count; ++k) {
        const DevicePtr* q = d + 16 * k;
        for (int c = 0; ok && c < 7; ++c)
            if (nodes[7 * k + c]) ok = CopyData2DtoDevice(*nodes[7 * k + c], q[c], H, dev_container_size_.pitch);
        steps[k] = {q[0], q[1], q[2], q[3], q[4], q[5], 0, q[6]};
        for (int c = 0; c < 9; ++c) out[9 * k + c] = q[7 + c];
    }
    const DevicePtr* diag = diagnostics ? d + 16 * step_count : nullptr;
    ok = ok && NodeStrainDevice(steps.data(), step_count, nw, nh, spacing, strain, planes ? out.data() : nullptr, stats_out, diag);
    // (without a record the device call only queues: the downloads below are ordered behind it on the stream)
    for (size_t k = 0; ok && planes && k < 9 * step_count; ++k)
        if (planes[k]) ok = CopyData2DFromDevice(out[k], *planes[k], H, dev_container_size_.pitch);
    for (size_t k = 0; ok && diagnostics && k < 3 * step_count; ++k)
        if (diagnostics[k]) ok = CopyData2DFromDevice(diag[k], *diagnostics[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::NodeStrainDevice(const SubsetPlanes* steps, size_t step_count, size_t nw, size_t nh, int spacing,
                                     const StrainOptions& strain, const DevicePtr* uncertainty, const DevicePtr* out_planes,
                                     flow2d_deformation_stats* stats_out, const DevicePtr* diagnostics,
                                     const StrainSigmaPlanes* strain_sigmas)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!StrainOptionsOk(strain)) return false;
    if (!strain.weighted) {
        std::printf("Error: '%s': the nodes' sigma planes go with weighted node strain.\n", GetName());
        return false;
    }
    if (!IsInitialized() || !steps || step_count == 0 || (!out_planes && !stats_out && !diagnostics && !strain_sigmas)) return false;
    if (nw == 0 || nh == 0 || nw > W || nh > H) {
        std::printf("Error: '%s': a %zu x %zu node grid does not lie in planes of %zu x %zu.\n", GetName(), nw, nh, W, H);
        return false;
    }
    if (RefuseGroup("node strain")) return false;
    for (size_t k = 0; k < step_count; ++k) {
        if (!steps[k].u || !steps[k].v || !uncertainty || !uncertainty[2 * k] || !uncertainty[2 * k + 1]) {
            std::printf("Error: '%s': step %zu of weighted node strain needs u, v, sigma_u and sigma_v.\n", GetName(), k + 1);
            return false;
        }
    }
    const int min_nodes = strain.min_nodes == 0 ? (strain.order == 2 ? 6 : 3) + 1 : strain.min_nodes;
    const int passes = strain.weight_threshold > 0.f ? strain.robust_iterations : 0;
    const size_t workspace_bytes = stats_out ? flow2d_node_strain_weighted_workspace_bytes(nw, nh, 1) : 0;
    const size_t per_step = sizeof(flow2d_deformation_stats) + workspace_bytes;
    if (stats_out && !strain_scratch_.Ensure(context_, step_count * per_step)) return false;
    auto plane = [](DevicePtr p) { return p ? AsPlane(p) : nullptr; };
    bool ok = true;
    for (size_t k = 0; ok && k < step_count; ++k) {
        const SubsetPlanes& q = steps[k];
        flow2d_deformation_planes out = {};
        if (out_planes) {
            const DevicePtr* d = out_planes + 9 * k;
            out = {plane(d[0]), plane(d[1]), plane(d[2]), plane(d[3]), plane(d[4]), plane(d[5]), plane(d[6]), plane(d[7]), plane(d[8])};
        }
        flow2d_node_strain_diagnostics diag = {};
        if (diagnostics) diag = {plane(diagnostics[3 * k]), plane(diagnostics[3 * k + 1]), plane(diagnostics[3 * k + 2])};
        flow2d_strain_sigma_planes sig = {};
        if (strain_sigmas) {
            const StrainSigmaPlanes& e = strain_sigmas[k];
            sig = {plane(e.sigma_ux),         plane(e.sigma_uy),        plane(e.sigma_vx),  plane(e.sigma_vy), plane(e.sigma_divergence),
                   plane(e.sigma_vorticity), plane(e.sigma_exx),       plane(e.sigma_eyy), plane(e.sigma_exy)};
        }
        auto* record = stats_out ? strain_scratch_.At<flow2d_deformation_stats>(k * per_step) : nullptr;
        void* workspace = stats_out ? strain_scratch_.At<>(k * per_step + sizeof(flow2d_deformation_stats)) : nullptr;
        // (the node planes are containers: the frames' pitch; the entry refuses planes that meet)
        ok = !CheckFlow2DError(flow2d_node_strain_weighted_2d(context_, AsPlane(q.u), AsPlane(q.v), plane(q.state), AsPlane(uncertainty[2 * k]),
                                                              AsPlane(uncertainty[2 * k + 1]), nw, nh, pitch, spacing, strain.window,
                                                              strain.order, min_nodes, strain.min_state, strain.measure, strain.sigma_floor,
                                                              strain.weight_threshold, passes, &out, &diag, &sig, record, workspace,
                                                              workspace_bytes),
                               "flow2d_node_strain_weighted_2d");
        if (ok && stats_out) ok = ReadRecord(stats_out + k, record, sizeof(*record));
    }
    if (!stats_out) return ok;
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::NodeStrain(Data2D* const* nodes, size_t step_count, int spacing, const StrainOptions& strain,
                               Data2D* const* uncertainty, Data2D* const* planes, flow2d_deformation_stats* stats_out,
                               Data2D* const* diagnostics, Data2D* const* strain_sigmas)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !nodes || step_count == 0 || !nodes[0] || !uncertainty ||
        (!planes && !stats_out && !diagnostics && !strain_sigmas) || !StrainOptionsOk(strain))
        return;
    if (!strain.weighted) {
        std::printf("Error: '%s': the nodes' sigma planes go with weighted node strain.\n", GetName());
        return;
    }
    const size_t nw = nodes[0]->Width(), nh = nodes[0]->Height(), H = dev_container_size_.height;
    if (nw == 0 || nh == 0 || nw > dev_container_size_.width || nh > H) {
        std::printf("Error: '%s': a %zu x %zu node grid does not lie in planes of %zu x %zu.\n", GetName(), nw, nh,
                    dev_container_size_.width, H);
        return;
    }
    // per step: u, v, state, sigma_u, sigma_v read (the gradients are not: a window fit), then 9 + 3 + 9 written
    constexpr int kIn = 5, kOut = 21, kPer = kIn + kOut;
    std::vector<Data2D*> images(kPer * step_count, nullptr);
    for (size_t k = 0; k < step_count; ++k) {
        Data2D** q = images.data() + kPer * k;
        q[0] = nodes[7 * k];
        q[1] = nodes[7 * k + 1];
        q[2] = nodes[7 * k + 6];
        q[3] = uncertainty[2 * k];
        q[4] = uncertainty[2 * k + 1];
        if (!q[0] || !q[1] || !q[3] || !q[4]) {
            std::printf("Error: '%s': step %zu of weighted node strain needs u, v, sigma_u and sigma_v.\n", GetName(), k + 1);
            return;
        }
        for (int c = 0; c < 9; ++c) q[kIn + c] = planes ? planes[9 * k + c] : nullptr;
        for (int c = 0; c < 3; ++c) q[kIn + 9 + c] = diagnostics ? diagnostics[3 * k + c] : nullptr;
        for (int c = 0; c < 9; ++c) q[kIn + 12 + c] = strain_sigmas ? strain_sigmas[9 * k + c] : nullptr;
        for (int c = 0; c < kPer; ++c)
            if (q[c] && (q[c]->Width() != nw || q[c]->Height() != nh)) {
                std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
                return;
            }
    }
    // the node planes, read and written: containers with no image of their size behind them, uploaded and downloaded here
    CallPlanes call_planes(context_, dev_container_size_, GetName(), "node");
    for (Data2D* image : images) call_planes.Add(nullptr, CallPlanes::Out, image != nullptr);
    HostCall call(context_, last_total_ms_, call_planes.Allocate());
    const DevicePtr* d = call_planes.data();
    bool ok = call_planes.Upload();
    std::vector<SubsetPlanes> steps(step_count);
    std::vector<DevicePtr> sigma_in(2 * step_count, 0), out(9 * step_count, 0), diag(3 * step_count, 0);
    std::vector<StrainSigmaPlanes> sig(step_count);
    for (size_t k = 0; k < step_count; ++k) {
        const DevicePtr* q = d + kPer * k;
        for (int c = 0; ok && c < kIn; ++c)
            if (images[kPer * k + c]) ok = CopyData2DtoDevice(*images[kPer * k + c], q[c], H, dev_container_size_.pitch);
        steps[k] = {q[0], q[1], 0, 0, 0, 0, 0, q[2]};
        sigma_in[2 * k] = q[3];
        sigma_in[2 * k + 1] = q[4];
        for (int c = 0; c < 9; ++c) out[9 * k + c] = q[kIn + c];
        for (int c = 0; c < 3; ++c) diag[3 * k + c] = q[kIn + 9 + c];
        const DevicePtr* e = q + kIn + 12;
        sig[k] = {e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7], e[8]};
    }
    ok = ok && NodeStrainDevice(steps.data(), step_count, nw, nh, spacing, strain, sigma_in.data(), planes ? out.data() : nullptr, stats_out,
                                diagnostics ? diag.data() : nullptr, strain_sigmas ? sig.data() : nullptr);
    // (without a record the device call only queues: the downloads below are ordered behind it on the stream)
    for (size_t k = 0; ok && k < step_count; ++k)
        for (int c = kIn; ok && c < kPer; ++c)
            if (images[kPer * k + c]) ok = CopyData2DFromDevice(d[kPer * k + c], *images[kPer * k + c], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::CorrelateSubsetSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, float lo, float scale,
                                                  const CorrelationPass* passes, size_t count, float min_score,
                                                  const ValidationOptions& validation, const SubsetOptions& subset,
                                                  const SequenceOptions& sequence, const SubsetPlanes* out,
                                                  CorrelationPassReport* first_reports, SequenceStepReport* steps_out,
                                                  const DevicePtr* dev_flows, flow2d_compose_record* compose_out)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!CorrelationPassesOk(W, H, lo, scale, passes, count, min_score, validation) || !SubsetOptionsOk(subset) ||
        !SequenceOptionsOk(sequence))
        return false;
    if (!IsInitialized() || !dev_frames || frame_count < 2 || !out) return false;
    if (RefuseGroup("a subset sequence")) return false;
    const size_t steps = frame_count - 1;
    const size_t every = static_cast<size_t>(sequence.reference_every);
    if (every > 0 && subset.mask) {
        std::printf("Error: '%s': a subset mask lies in frame 0's coordinates, and with a new reference frame every %zu steps the later "
                    "references' subsets do not: a moving reference takes no mask.\n",
                    GetName(), every);
        return false;
    }
    for (size_t k = 0; every > 0 && k < steps; ++k)
        if (out[k].uxx || out[k].uxy || out[k].uyy || out[k].vxx || out[k].vxy || out[k].vyy) {
            std::printf("Error: '%s': with a moving reference the delivered fields are compositions, which know gradients only: step %zu "
                        "takes no curvature planes.\n",
                        GetName(), k + 1);
            return false;
        }
    {
        // every step's planes are the next step's input and pass through the prediction, which knows no frame: checked here
        std::vector<DevicePtr> written;
        for (size_t k = 0; k < steps; ++k) {
            const SubsetPlanes& o = out[k];
            if (!o.u || !o.v || !o.ux || !o.uy || !o.vx || !o.vy || !o.state) {
                std::printf("Error: '%s': step %zu of a subset sequence needs u, v, the four gradients and the state.\n", GetName(), k + 1);
                return false;
            }
            for (DevicePtr p : {o.u, o.v, o.ux, o.uy, o.vx, o.vy, o.score, o.state, o.uxx, o.uxy, o.uyy, o.vxx, o.vxy, o.vyy})
                if (p) written.push_back(p);
            if (dev_flows && (dev_flows[2 * k] == 0) != (dev_flows[2 * k + 1] == 0)) return false;
            for (int c = 0; dev_flows && c < 2; ++c)
                if (dev_flows[2 * k + c]) written.push_back(dev_flows[2 * k + c]);
        }
        if (!WrittenPlanesOk(dev_frames, frame_count, written.data(), written.size(), "node or flow plane")) return false;
    }
    if (!EnsurePlanes(sequence_planes_, 14)) return false;
    const size_t per_step = sizeof(flow2d_subset_record) + kSequenceMaxFill * sizeof(flow2d_predict_record);
    // (with a moving reference the compositions' records lie behind the steps')
    if (!sequence_scratch_.Ensure(context_, steps * per_step + (every > 0 && compose_out ? steps * sizeof(flow2d_compose_record) : 0)))
        return false;
    if (every > 0 && every < steps && !EnsurePlanes(reference_planes_, 23)) return false;
    const CorrelationPass& fine = passes[count - 1];
    if (steps_out) std::fill(steps_out, steps_out + steps, SequenceStepReport{});
    if (compose_out) std::fill(compose_out, compose_out + steps, flow2d_compose_record{});
    // step 1: the pair chain
    bool ok = QueueCorrelateSubset(dev_frames[0], dev_frames[1], lo, scale, passes, count, min_score, validation, subset, 0, 0, out[0],
                                   first_reports, steps_out ? &steps_out[0].subset : nullptr, dev_flows ? dev_flows[0] : 0,
                                   dev_flows ? dev_flows[1] : 0, false);
    SubsetOptions later = subset;
    later.max_shift = sequence.max_shift;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(W, H, fine.radius, fine.spacing, &nw, &nh);
    auto set_of = [](const DevicePtr* d) { return SubsetPlanes{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]}; };
    int written = 0;  // the set of reference_planes_ the last increment lies in
    for (size_t k = 1; ok && k < steps; ++k) {
        const size_t ref = every > 0 ? every * (k / every) : 0;  // step k + 1 against frame ref
        SequenceStepReport* report = steps_out ? &steps_out[k] : nullptr;
        const DevicePtr flow_u = dev_flows ? dev_flows[2 * k] : 0, flow_v = dev_flows ? dev_flows[2 * k + 1] : 0;
        if (ref == 0) {
            ok = QueueSequenceStep(dev_frames[0], dev_frames[k + 1], out[k - 1], fine.radius, fine.spacing, later, sequence, out[k], report,
                                   k * per_step, flow_u, flow_v);
            continue;
        }
        const DevicePtr* base = reference_planes_.data() + 16;
        const SubsetPlanes increment = set_of(reference_planes_.data() + 8 * (written ^ 1));
        if (ref == k) {
            // the reference moves to frame `ref`: its base is the delivered field of step `ref`, refilled, the last pass into the
            // base's planes; then the pair chain from the new reference
            const SubsetPlanes& field = out[ref - 1];
            const float* in[7] = {AsPlane(field.u),  AsPlane(field.v),  AsPlane(field.ux),   AsPlane(field.uy),
                                  AsPlane(field.vx), AsPlane(field.vy), AsPlane(field.state)};
            for (int pass = 0; ok && pass < sequence.fill; ++pass) {
                const DevicePtr* set = pass == sequence.fill - 1 ? base : sequence_planes_.data() + 7 * (pass & 1);
                auto* record = sequence_scratch_.At<flow2d_predict_record>(k * per_step + sizeof(flow2d_subset_record) +
                                                                            pass * sizeof(flow2d_predict_record));
                ok = !CheckFlow2DError(flow2d_predict_nodes_2d(context_, in[0], in[1], in[2], in[3], in[4], in[5], in[6], nw, nh, pitch,
                                                               fine.spacing, sequence.min_state, sequence.min_neighbours, AsPlane(set[0]),
                                                               AsPlane(set[1]), AsPlane(set[2]), AsPlane(set[3]), AsPlane(set[4]),
                                                               AsPlane(set[5]), AsPlane(set[6]), report ? record : nullptr),
                                       "flow2d_predict_nodes_2d");
                if (ok && report) ok = ReadRecord(&report->prediction[pass], record, sizeof(*record));
                for (int c = 0; c < 7; ++c) in[c] = AsPlane(set[c]);
            }
            ok = ok && QueueCorrelateSubset(dev_frames[ref], dev_frames[k + 1], lo, scale, passes, count, min_score, validation, subset, 0, 0,
                                            increment, nullptr, report ? &report->subset : nullptr, 0, 0, false);
        } else {
            ok = QueueSequenceStep(dev_frames[ref], dev_frames[k + 1], set_of(reference_planes_.data() + 8 * written), fine.radius,
                                   fine.spacing, later, sequence, increment, report, k * per_step, 0, 0);
        }
        written ^= 1;
        auto* record = compose_out ? sequence_scratch_.At<flow2d_compose_record>(steps * per_step + k * sizeof(flow2d_compose_record)) : nullptr;
        ok = ok && QueueComposeNodes(SubsetPlanes{base[0], base[1], base[2], base[3], base[4], base[5], 0, base[6]}, increment, fine.radius,
                                     fine.spacing, sequence.min_state, out[k], record);
        if (ok && compose_out) ok = ReadRecord(compose_out + k, record, sizeof(*record));
        if (ok && flow_u)
            ok = !CheckFlow2DError(flow2d_expand_nodes_2d(context_, AsPlane(out[k].u), AsPlane(out[k].v), nw, nh, pitch, fine.radius,
                                                          fine.spacing, AsPlane(flow_u), AsPlane(flow_v), W, H, pitch),
                                   "flow2d_expand_nodes_2d");
    }
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

bool OpticalFlow2D::QueueComposeNodes(const SubsetPlanes& base, const SubsetPlanes& increment, int grid_radius, int spacing, int min_state,
                                      const SubsetPlanes& out, flow2d_compose_record* record)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(W, H, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) {
        std::printf("Error: a %zu x %zu frame holds no node grid of radius %d and spacing %d.\n", W, H, grid_radius, spacing);
        return false;
    }
    auto plane = [](DevicePtr p) { return p ? AsPlane(p) : nullptr; };
    // (the node planes are containers: the frames' pitch; the entry refuses planes that meet)
    const float* const a[7] = {plane(base.u), plane(base.v), plane(base.ux), plane(base.uy), plane(base.vx), plane(base.vy), plane(base.state)};
    const float* const b[7] = {plane(increment.u),  plane(increment.v),  plane(increment.ux),   plane(increment.uy),
                               plane(increment.vx), plane(increment.vy), plane(increment.state)};
    float* const o[6] = {plane(out.u), plane(out.v), plane(out.ux), plane(out.uy), plane(out.vx), plane(out.vy)};
    return !CheckFlow2DError(flow2d_compose_nodes_2d(context_, a, b, out.score ? plane(increment.score) : nullptr, nw, nh, pitch, grid_radius,
                                                     spacing, min_state, o, plane(out.state), plane(out.score), record),
                             "flow2d_compose_nodes_2d");
}

bool OpticalFlow2D::ComposeNodesDevice(const SubsetPlanes& base, const SubsetPlanes& increment, int grid_radius, int spacing, int min_state,
                                       const SubsetPlanes& out, flow2d_compose_record* record_out)
{
    if (!IsInitialized()) return false;
    if (min_state != 0 && min_state != 1) {
        std::printf("Error: '%s': a composition takes a least state of 0 or 1 (%d).\n", GetName(), min_state);
        return false;
    }
    for (const SubsetPlanes* q : {&base, &increment})
        if (!q->u || !q->v || !q->ux || !q->uy || !q->vx || !q->vy || !q->state) {
            std::printf("Error: '%s': base and increment of a composition need u, v, the four gradients and the state.\n", GetName());
            return false;
        }
    if (!out.u || !out.v || !out.ux || !out.uy || !out.vx || !out.vy || (out.score && !increment.score) || out.uxx || out.uxy || out.uyy ||
        out.vxx || out.vxy || out.vyy) {
        std::printf("Error: '%s': a composition writes u, v and the four gradients, a score only from the increment's, and no "
                    "curvatures.\n",
                    GetName());
        return false;
    }
    if (RefuseGroup("a composition of node fields")) return false;
    if (record_out && !compose_scratch_.Ensure(context_, sizeof(flow2d_compose_record))) return false;
    flow2d_compose_record* record = record_out ? compose_scratch_.At<flow2d_compose_record>() : nullptr;
    bool ok = QueueComposeNodes(base, increment, grid_radius, spacing, min_state, out, record);
    if (!ok || !record_out) return ok;
    ok = ReadRecord(record_out, record, sizeof(*record_out));
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::ComposeNodes(Data2D* const* base, Data2D* const* increment, int grid_radius, int spacing, int min_state,
                                 Data2D* const* nodes, flow2d_compose_record* record_out)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !base || !increment || !nodes) return;
    for (int k = 0; k < 7; ++k)
        if (!base[k] || (k != 6 && !increment[k]) || (k < 6 && !nodes[k])) return;
    if (!increment[7] || (nodes[6] && !increment[6])) return;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(W, H, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) {
        std::printf("Error: a %zu x %zu frame holds no node grid of radius %d and spacing %d.\n", W, H, grid_radius, spacing);
        return;
    }
    for (int k = 0; k < 23; ++k) {
        Data2D* image = k < 7 ? base[k] : (k < 15 ? increment[k - 7] : nodes[k - 15]);
        if (image && (image->Width() != nw || image->Height() != nh)) {
            std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
            return;
        }
    }
    // the node planes, read and written: containers with no image of their size behind them, uploaded and downloaded here
    CallPlanes planes(context_, dev_container_size_, GetName(), "node");
    for (int k = 0; k < 7; ++k) planes.Add(nullptr, CallPlanes::Out, true);
    for (int k = 0; k < 8; ++k) planes.Add(nullptr, CallPlanes::Out, increment[k] != nullptr);
    for (int k = 0; k < 8; ++k) planes.Add(nullptr, CallPlanes::Out, nodes[k] != nullptr);
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    bool ok = planes.Upload();
    for (int k = 0; ok && k < 7; ++k) ok = CopyData2DtoDevice(*base[k], d[k], H, dev_container_size_.pitch);
    for (int k = 0; ok && k < 8; ++k)
        if (increment[k]) ok = CopyData2DtoDevice(*increment[k], d[7 + k], H, dev_container_size_.pitch);
    const SubsetPlanes a = {d[0], d[1], d[2], d[3], d[4], d[5], 0, d[6]};
    ok = ok && ComposeNodesDevice(a, NodePlanes(d + 7, 8), grid_radius, spacing, min_state, NodePlanes(d + 15, 8), record_out);
    // (without a record the device call only queues: the downloads below are ordered behind it on the stream)
    for (int k = 0; ok && k < 8; ++k)
        if (nodes[k]) ok = CopyData2DFromDevice(d[15 + k], *nodes[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::UncertaintyOptionsOk(const SubsetOptions& subset, int min_state)
{
    if (subset.order == 2) {
        std::printf("Error: the node uncertainty is that of the first-order refinement: twelve parameters need a 12 x 12 covariance, "
                    "which is not built here (order %d).\n",
                    subset.order);
        return false;
    }
    if (!SubsetOptionsOk(subset)) return false;
    if (min_state != 0 && min_state != 1) {
        std::printf("Error: the node uncertainty takes a least state of 0 or 1 (%d).\n", min_state);
        return false;
    }
    return true;
}

bool OpticalFlow2D::NodeUncertaintyDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, const SubsetPlanes& nodes, int grid_radius,
                                          int spacing, const SubsetOptions& subset, int min_state, const UncertaintyPlanes& out,
                                          flow2d_uncertainty_record* record_out)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!UncertaintyOptionsOk(subset, min_state)) return false;
    if (nodes.uxx || nodes.uxy || nodes.uyy || nodes.vxx || nodes.vxy || nodes.vyy) {
        std::printf("Error: '%s': the node uncertainty takes no curvature planes: twelve parameters need a 12 x 12 covariance, which is "
                    "not built here.\n",
                    GetName());
        return false;
    }
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(W, H, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) {
        std::printf("Error: a %zu x %zu frame holds no node grid of radius %d and spacing %d.\n", W, H, grid_radius, spacing);
        return false;
    }
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1) return false;
    if (!nodes.u || !nodes.v || !nodes.ux || !nodes.uy || !nodes.vx || !nodes.vy || !nodes.state) {
        std::printf("Error: '%s': the node uncertainty needs u, v, the four gradients and the state of a refinement.\n", GetName());
        return false;
    }
    const bool gradients = out.sigma_ux != 0;
    if (!out.sigma_u || !out.sigma_v || (out.sigma_uy != 0) != gradients || (out.sigma_vx != 0) != gradients ||
        (out.sigma_vy != 0) != gradients) {
        std::printf("Error: '%s': the node uncertainty writes sigma_u and sigma_v, and the four gradient sigmas all or none.\n", GetName());
        return false;
    }
    if (RefuseGroup("the node uncertainty")) return false;
    if (record_out && !uncertainty_scratch_.Ensure(context_, sizeof(flow2d_uncertainty_record))) return false;
    flow2d_uncertainty_record* record = record_out ? uncertainty_scratch_.At<flow2d_uncertainty_record>() : nullptr;
    auto plane = [](DevicePtr p) { return p ? AsPlane(p) : nullptr; };
    const bool spline = subset.interpolation == SubsetOptions::BSpline;
    if (spline) {
        // frame 1's coefficients, on the same stream in front of the kernel that samples them
        if (!EnsurePlanes(spline_plane_, 1) ||
            CheckFlow2DError(flow2d_bspline_prefilter_2d(context_, AsPlane(dev_frame_1), AsPlane(spline_plane_[0]), W, H, pitch),
                             "flow2d_bspline_prefilter_2d"))
            return false;
    }
    // (the node planes are containers: the frames' pitch; the entry refuses planes that meet)
    bool ok = !CheckFlow2DError(
        flow2d_subset_uncertainty_2d(context_, AsPlane(dev_frame_0), AsPlane(spline ? spline_plane_[0] : dev_frame_1), spline ? 1 : 0, W, H,
                                     pitch, AsPlane(nodes.u), AsPlane(nodes.v), AsPlane(nodes.ux), AsPlane(nodes.uy), AsPlane(nodes.vx),
                                     AsPlane(nodes.vy), AsPlane(nodes.state), nw, nh, pitch, grid_radius, spacing, subset.radius, min_state,
                                     plane(subset.mask), SubsetMinPixels(subset), AsPlane(out.sigma_u), AsPlane(out.sigma_v), plane(out.rho),
                                     plane(out.sigma_ux), plane(out.sigma_uy), plane(out.sigma_vx), plane(out.sigma_vy), plane(out.noise),
                                     record),
        "flow2d_subset_uncertainty_2d");
    if (!ok || !record_out) return ok;
    ok = ReadRecord(record_out, record, sizeof(*record_out));
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::NodeUncertainty(Data2D& frame_0, Data2D& frame_1, Data2D* const* nodes, int grid_radius, int spacing,
                                    const SubsetOptions& subset, int min_state, Data2D* const* out, flow2d_uncertainty_record* record_out,
                                    Data2D* mask)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !nodes || !out || !out[0] || !out[1]) return;
    for (int k = 0; k < 8; ++k)
        if (k != 6 && !nodes[k]) return;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(W, H, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) {
        std::printf("Error: a %zu x %zu frame holds no node grid of radius %d and spacing %d.\n", W, H, grid_radius, spacing);
        return;
    }
    for (int k = 0; k < 16; ++k) {
        Data2D* image = k < 8 ? (k == 6 ? nullptr : nodes[k]) : out[k - 8];
        if (image && (image->Width() != nw || image->Height() != nh)) {
            std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
            return;
        }
    }
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In);
    // the node planes, read and written: containers with no image of their size behind them, uploaded and downloaded here
    for (int k = 0; k < 8; ++k) planes.Add(nullptr, CallPlanes::Out, k != 6);
    for (int k = 0; k < 8; ++k) planes.Add(nullptr, CallPlanes::Out, out[k] != nullptr);
    if (mask) planes.Add(mask, CallPlanes::In);  // behind everything else
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    bool ok = planes.Upload();
    for (int k = 0; ok && k < 8; ++k)
        if (k != 6) ok = CopyData2DtoDevice(*nodes[k], d[2 + k], H, dev_container_size_.pitch);
    SubsetPlanes field;
    field = {d[2], d[3], d[4], d[5], d[6], d[7], 0, d[9]};
    const UncertaintyPlanes planes_out = {d[10], d[11], d[12], d[13], d[14], d[15], d[16], d[17]};
    SubsetOptions masked = subset;
    masked.mask = mask ? d[18] : 0;
    ok = ok && NodeUncertaintyDevice(d[0], d[1], field, grid_radius, spacing, masked, min_state, planes_out, record_out);
    // (without a record the device call only queues: the downloads below are ordered behind it on the stream)
    for (int k = 0; ok && k < 8; ++k)
        if (out[k]) ok = CopyData2DFromDevice(d[10 + k], *out[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

void OpticalFlow2D::CorrelateSubsetSequence(Data2D* const* frames, size_t frame_count, const CorrelationPass* passes, size_t count,
                                            float min_score, const ValidationOptions& validation, const SubsetOptions& subset,
                                            const SequenceOptions& sequence, Data2D* const* nodes, CorrelationPassReport* first_reports,
                                            SequenceStepReport* steps_out, Data2D* const* flows, Data2D* mask,
                                            flow2d_compose_record* compose_out)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !frames || frame_count < 2 || !nodes) return;
    const size_t steps = frame_count - 1, images = static_cast<size_t>(NodeImages(subset));
    for (size_t k = 0; k < frame_count; ++k)
        if (!frames[k]) return;
    for (size_t k = 0; k < steps; ++k) {
        for (int c = 0; c < 8; ++c)
            if (c != 6 && !nodes[images * k + c]) return;
        if (!CurvatureImagesOk(nodes + images * k, static_cast<int>(images))) return;
        if (flows && (flows[2 * k] == nullptr) != (flows[2 * k + 1] == nullptr)) return;
    }
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    for (size_t k = 0; k < frame_count; ++k) planes.Add(frames[k], CallPlanes::In);
    for (size_t k = 0; k < 2 * steps; ++k) planes.Add(flows ? flows[k] : nullptr, CallPlanes::Out);
    // the node planes: containers with no image of their size behind them, downloaded below
    for (size_t k = 0; k < images * steps; ++k) planes.Add(nullptr, CallPlanes::Out, nodes[k] != nullptr);
    if (mask) planes.Add(mask, CallPlanes::In);  // uploaded once for all steps, behind everything else
    if (!planes.SizesMatch()) return;
    float lo = 0.f, scale = 1.f;
    CorrelationRange(*frames[0], *frames[1], lo, scale);
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    SubsetOptions masked = subset;
    masked.mask = mask ? 1 : 0;  // (for the check; the plane's address below)
    if (!CorrelationPassesOk(W, H, lo, scale, passes, count, min_score, validation) || !SubsetOptionsOk(masked) ||
        !SequenceOptionsOk(sequence))
        return;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(W, H, passes[count - 1].radius, passes[count - 1].spacing, &nw, &nh);
    for (size_t k = 0; k < images * steps; ++k)
        if (nodes[k] && (nodes[k]->Width() != nw || nodes[k]->Height() != nh)) {
            std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
            return;
        }
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    const DevicePtr* dev_flows = d + frame_count;
    const DevicePtr* dev_nodes = dev_flows + 2 * steps;
    std::vector<SubsetPlanes> out(steps);
    for (size_t k = 0; k < steps; ++k) {
        out[k] = NodePlanes(dev_nodes + images * k, static_cast<int>(images));
    }
    masked.mask = mask ? dev_nodes[images * steps] : 0;
    bool ok = planes.Upload() &&
              CorrelateSubsetSequenceDevice(d, frame_count, lo, scale, passes, count, min_score, validation, masked, sequence, out.data(),
                                            first_reports, steps_out, flows ? dev_flows : nullptr, compose_out) &&
              planes.Download();
    for (size_t k = 0; ok && k < images * steps; ++k)
        if (nodes[k]) ok = CopyData2DFromDevice(dev_nodes[k], *nodes[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

void OpticalFlow2D::CorrelateMultiPass(Data2D& frame_0, Data2D& frame_1, const CorrelationPass* passes, size_t count, float min_score,
                                       const ValidationOptions& validation, Data2D& node_u, Data2D& node_v, Data2D* node_score,
                                       CorrelationPassReport* reports_out, Data2D* flow_u, Data2D* flow_v, Data2D* predictor_u,
                                       Data2D* predictor_v, Data2D* mask)
{
    last_run_ok_ = false;
    if (!IsInitialized() || (flow_u == nullptr) != (flow_v == nullptr) || (predictor_u == nullptr) != (predictor_v == nullptr)) return;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In).Add(flow_u, CallPlanes::Out).Add(flow_v, CallPlanes::Out);
    // the node planes: containers with no image of their size behind them, downloaded below
    planes.Add(nullptr, CallPlanes::Out, true).Add(nullptr, CallPlanes::Out, true).Add(nullptr, CallPlanes::Out, node_score != nullptr);
    if (predictor_u) planes.Add(predictor_u, CallPlanes::In).Add(predictor_v, CallPlanes::In);
    const int mask_at = 7 + (predictor_u ? 2 : 0);  // the mask, uploaded once, behind everything else
    if (mask) planes.Add(mask, CallPlanes::In);
    if (!planes.SizesMatch()) return;
    float lo = 0.f, scale = 1.f;
    CorrelationRange(frame_0, frame_1, lo, scale);
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    if (!CorrelationPassesOk(W, H, lo, scale, passes, count, min_score, validation)) return;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(W, H, passes[count - 1].radius, passes[count - 1].spacing, &nw, &nh);
    Data2D* nodes[3] = {&node_u, &node_v, node_score};
    for (Data2D* image : nodes)
        if (image && (image->Width() != nw || image->Height() != nh)) {
            std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
            return;
        }
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    ValidationOptions masked = validation;
    masked.mask = mask ? d[mask_at] : 0;
    bool ok = planes.Upload() &&
              CorrelateMultiPassDevice(d[0], d[1], lo, scale, passes, count, min_score, masked, predictor_u ? d[7] : 0, predictor_u ? d[8] : 0, d[4],
                                       d[5], d[6],
                                       reports_out, d[2], d[3]) &&
              planes.Download();
    for (int k = 0; ok && k < 3; ++k)
        if (nodes[k]) ok = CopyData2DFromDevice(d[4 + k], *nodes[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::StabiliseSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, size_t reference_index, int model,
                                            double sigma, int iterations, bool use_masks, float fill,
                                            const DevicePtr* dev_outputs, flow2d_global_motion* motions_out,
                                            OperationParameters& params)
{
    if (!GlobalMotionArgsOk(model, sigma, iterations)) return false;
    if (frame_count < 2 || reference_index >= frame_count) {
        std::printf("Error: stabilisation takes at least 2 frames (%zu) and a reference frame among them (%zu).\n", frame_count,
                    reference_index);
        return false;
    }
    if (!IsInitialized() || !dev_frames || !dev_outputs) return false;
    if (RefuseGroup("sequences")) return false;
    if (!WrittenPlanesOk(dev_frames, frame_count, dev_outputs, frame_count, "output plane")) return false;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const size_t ref = reference_index;
    // steps[k]: above the reference M(k - 1 -> k), below it M(k + 1 -> k)
    std::vector<flow2d_global_motion> steps(frame_count), composed(frame_count);
    std::vector<DevicePtr> reversed(dev_frames, dev_frames + ref + 1);
    std::reverse(reversed.begin(), reversed.end());  // frame ref, ref - 1, ..., 0
    std::vector<flow2d_global_motion> below(ref);
    if (!FitConsecutivePairs(dev_frames + ref, frame_count - ref, model, sigma, iterations, use_masks, steps.data() + ref + 1, params) ||
        !FitConsecutivePairs(reversed.data(), ref + 1, model, sigma, iterations, use_masks, below.data(), params))
        return false;
    for (size_t i = 0; i < ref; ++i) steps[ref - 1 - i] = below[i];
    flow2d_global_motion identity = {};
    identity.model_used = model;
    composed[ref] = identity;
    for (size_t k = ref + 1; k < frame_count; ++k)
        composed[k] = k == ref + 1 ? steps[k] : ComposeGlobalMotion(composed[k - 1], steps[k]);
    for (size_t k = ref; k-- > 0;) composed[k] = k + 1 == ref ? steps[k] : ComposeGlobalMotion(composed[k + 1], steps[k]);
    if (!EnsureStabiliseScratch()) return false;
    bool ok = true;
    for (size_t k = 0; ok && k < frame_count; ++k) {
        if (k == ref) {
            ok = HandBack(1, dev_frames + k, dev_outputs + k);
            continue;
        }
        // (one record slot: the upload of the next record is ordered behind this warp on the stream)
        ok = !CheckFlow2DError(flow2d_copy_h2d_2d(context_, StabiliseRecord(kStabiliseWindow), sizeof(flow2d_global_motion), &composed[k],
                                                  sizeof(flow2d_global_motion), sizeof(flow2d_global_motion), 1),
                               "flow2d_copy_h2d_2d") &&
             !CheckFlow2DError(flow2d_warp_global_2d(context_, StabiliseRecord(kStabiliseWindow), AsPlane(dev_frames[k]), W, H, pitch,
                                                     fill, AsPlane(dev_outputs[k]), nullptr),
                               "flow2d_warp_global_2d");
    }
    ok = !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;  // `composed` is the uploads' source
    if (ok && motions_out)
        for (size_t k = 0; k < frame_count; ++k) motions_out[k] = composed[k];
    return ok;
}

void OpticalFlow2D::StabiliseSequence(Data2D* const* frames, size_t frame_count, size_t reference_index, int model, double sigma,
                                      int iterations, bool use_masks, float fill, Data2D* outputs,
                                      flow2d_global_motion* motions_out, OperationParameters& params)
{
    last_run_ok_ = false;
    if (!GlobalMotionArgsOk(model, sigma, iterations)) return;
    if (!IsInitialized() || !frames || !outputs || frame_count < 2 || reference_index >= frame_count) return;
    const size_t n = frame_count;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / output");
    planes.Add(frames, n, CallPlanes::In).Add(outputs, n, CallPlanes::Out);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    last_run_ok_ = planes.Upload() &&
                   StabiliseSequenceDevice(d, n, reference_index, model, sigma, iterations, use_masks, fill, d + n, motions_out, params) &&
                   planes.Download();
}

bool OpticalFlow2D::DenoiseArgsOk(size_t frame_count, size_t radius, float range_sigma)
{
    if (frame_count < 2 || radius < 1 || radius > kDenoiseMaxRadius || !std::isfinite(range_sigma) || range_sigma < 0.f) {
        std::printf("Error: denoising takes at least 2 frames (%zu), a radius of 1 .. %zu (%zu) and a finite range sigma >= 0 (%g).\n",
                    frame_count, kDenoiseMaxRadius, radius, range_sigma);
        return false;
    }
    return true;
}

bool OpticalFlow2D::DenoiseSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, size_t radius, float range_sigma,
                                          bool use_masks, const DevicePtr* dev_outputs, const DevicePtr* dev_weight_sums,
                                          OperationParameters& params)
{
    if (!DenoiseArgsOk(frame_count, radius, range_sigma)) return false;
    if (!IsInitialized() || !dev_frames || !dev_outputs) return false;
    if (RefuseGroup("sequences")) return false;
    // every plane written must be distinct from every other one and from the frames (which are only read)
    std::vector<DevicePtr> written(dev_outputs, dev_outputs + frame_count);
    if (dev_weight_sums) written.insert(written.end(), dev_weight_sums, dev_weight_sums + frame_count);
    if (!WrittenPlanesOk(dev_frames, frame_count, written.data(), written.size(), "output plane")) return false;
    // the ring: pair j lives in slot j % slots as u, v, back u, back v, occlusion forward, occlusion backward
    const size_t slots = 2 * radius + kDenoiseWindow;
    const size_t per_slot = use_masks ? 6 : 4;
    for (size_t s = 0; s < slots; ++s)
        if (!EnsurePlanes(&denoise_pairs_[6 * s], per_slot)) return false;
    // the composed flows of one centre: direction (0 backwards, 1 forwards), distance d >= 2: u, v, mask
    const size_t far = kDenoiseMaxRadius - 1;
    for (size_t dir = 0; dir < 2; ++dir)
        for (size_t d = 2; d <= radius; ++d)
            if (!EnsurePlanes(&denoise_chains_[(dir * far + d - 2) * 3], use_masks ? 3 : 2)) return false;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    auto pair_plane = [&](size_t j, size_t i) { return denoise_pairs_[6 * (j % slots) + i]; };
    auto chain_plane = [&](size_t dir, size_t d, size_t i) { return denoise_chains_[(dir * far + d - 2) * 3 + i]; };

    auto fuse = [&](size_t k) {
        // the flow from frame k to frame k -+ d and its mask: distance 1 from the ring, further ones chained outwards
        DevicePtr flow[2][kDenoiseMaxRadius][3];
        size_t reach[2] = {std::min(radius, k), std::min(radius, frame_count - 1 - k)};
        for (size_t dir = 0; dir < 2; ++dir) {
            for (size_t d = 1; d <= reach[dir]; ++d) {
                // the step that ends at distance d: backwards the backward flow of pair k - d, forwards the forward flow of
                // pair k + d - 1, each with the mask on its own first frame's grid
                const size_t j = dir ? k + d - 1 : k - d;
                const DevicePtr step[3] = {pair_plane(j, dir ? 0 : 2), pair_plane(j, dir ? 1 : 3),
                                           use_masks ? pair_plane(j, dir ? 4 : 5) : 0};
                if (d == 1) {
                    for (int i = 0; i < 3; ++i) flow[dir][0][i] = step[i];
                    continue;
                }
                DevicePtr* out = flow[dir][d - 1];
                for (int i = 0; i < 3; ++i) out[i] = (i < 2 || use_masks) ? chain_plane(dir, d, i) : 0;
                const DevicePtr* prev = flow[dir][d - 2];
                if (CheckFlow2DError(flow2d_compose_flow_2d(context_, AsPlane(prev[0]), AsPlane(prev[1]), AsPlane(step[0]),
                                                            AsPlane(step[1]), use_masks ? AsPlane(prev[2]) : nullptr,
                                                            use_masks ? AsPlane(step[2]) : nullptr, W, H, pitch, AsPlane(out[0]),
                                                            AsPlane(out[1]), use_masks ? AsPlane(out[2]) : nullptr),
                                     "flow2d_compose_flow_2d"))
                    return false;
            }
        }
        // ascending frame order: k - reach .. k - 1, k + 1 .. k + reach
        const float *frames[2 * kDenoiseMaxRadius], *us[2 * kDenoiseMaxRadius], *vs[2 * kDenoiseMaxRadius],
            *occs[2 * kDenoiseMaxRadius];
        size_t n = 0;
        auto add = [&](size_t dir, size_t d) {
            frames[n] = AsPlane(dev_frames[dir ? k + d : k - d]);
            us[n] = AsPlane(flow[dir][d - 1][0]);
            vs[n] = AsPlane(flow[dir][d - 1][1]);
            occs[n] = use_masks ? AsPlane(flow[dir][d - 1][2]) : nullptr;
            ++n;
        };
        for (size_t d = reach[0]; d >= 1; --d) add(0, d);
        for (size_t d = 1; d <= reach[1]; ++d) add(1, d);
        return !CheckFlow2DError(flow2d_denoise_2d(context_, AsPlane(dev_frames[k]), n, frames, us, vs, use_masks ? occs : nullptr, W,
                                                   H, pitch, range_sigma, AsPlane(dev_outputs[k]),
                                                   dev_weight_sums ? AsPlane(dev_weight_sums[k]) : nullptr),
                                 "flow2d_denoise_2d");
    };

    const size_t pairs = frame_count - 1;
    size_t done = 0, centre = 0;  // pairs in the ring so far; the next frame to fuse
    bool ok = true;
    while (ok && centre < frame_count) {
        if (done < pairs) {
            const size_t chunk = std::min(kDenoiseWindow, pairs - done);
            std::vector<DevicePtr> p[6];
            for (size_t j = done; j < done + chunk; ++j)
                for (size_t i = 0; i < 6; ++i) p[i].push_back(pair_plane(j, i));
            ok = ComputeFlowBidirectionalDevice(dev_frames + done, chunk + 1, p[0].data(), p[1].data(), p[2].data(), p[3].data(),
                                                use_masks ? p[4].data() : nullptr, use_masks ? p[5].data() : nullptr, params);
            done += chunk;
        }
        // every frame whose furthest forward pair is in the ring (a slot is overwritten only 2 * radius + kDenoiseWindow pairs later)
        while (ok && centre < frame_count && std::min(centre + radius, pairs) <= done) ok = fuse(centre++);
    }
    return ok;
}

void OpticalFlow2D::DenoiseSequence(Data2D* const* frames, size_t frame_count, size_t radius, float range_sigma, bool use_masks,
                                    Data2D* outputs, Data2D* weight_sums, OperationParameters& params)
{
    last_run_ok_ = false;
    if (!DenoiseArgsOk(frame_count, radius, range_sigma)) return;
    if (!IsInitialized() || !frames || !outputs) return;
    if (RefuseGroup("sequences")) return;
    const size_t n = frame_count;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / output");
    planes.Add(frames, n, CallPlanes::In).Add(outputs, n, CallPlanes::Out).Add(weight_sums, n, CallPlanes::Out);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    bool ok = planes.Upload() && DenoiseSequenceDevice(d, n, radius, range_sigma, use_masks, d + n, weight_sums ? d + 2 * n : nullptr, params);
    for (size_t k = 0; ok && k < n; ++k) ok = planes.Download(n + k) && planes.Download(2 * n + k);  // output k, then its sum of weights
    last_run_ok_ = ok;
}
