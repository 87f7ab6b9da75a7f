// C facade over the C++ host layer, for the Python tests and bench.py (plumbing only).
// It drives the same OpticalFlow2D / OperationParameters objects a C++ caller would.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <new>
#include <vector>

#include "device_utils.h"
#include "flow_evaluation.h"
#include "io_utils.h"
#include "optical_flow_2d.h"
#include "optical_flow_batch_2d.h"
#include "settings.h"

#define HOST_API extern "C" __attribute__((visibility("default")))

struct flow2d_host_params {
    size_t warp_levels_count;
    float warp_scale_factor;
    size_t outer_iterations_count;
    size_t inner_iterations_count;
    float equation_alpha;
    float equation_smoothness;
    float equation_data;
    size_t median_radius;
    float gaussian_sigma;
    int solver_algorithm;
    float sor_omega;
};

struct flow2d_host_flow {
    OpticalFlow2D flow;
    size_t width = 0, height = 0;
    int subset_interpolation = OpticalFlow2D::SubsetOptions::CatmullRom;  // flow2d_host_set_subset_interpolation
    bool subset_mask_search = false;                                      // flow2d_host_set_subset_mask_search
    int reference_every = 0;                                              // flow2d_host_set_reference_every
    float strain_sigma = 0.f;                                             // flow2d_host_set_strain_robust
    int strain_iterations = 8;
    bool strain_weighted = false;                                         // flow2d_host_set_strain_weighting
    float strain_floor = 0.f, strain_threshold = 0.f;
    int strain_weight_iterations = 0;
    std::vector<void*> strain_diagnostics;  // flow2d_host_set_strain_diagnostics: of the next node-strain call, which forgets them
    std::vector<flow2d_compose_record> compose_records;                   // of the last sequence call: flow2d_host_compose_records
};

namespace {
// The parameter bag of one call.  The bag holds pointers, so the object owns what they point to: a copy of the caller's block and,
// for the entries that take them, the consistency thresholds (the bag keys consistency_alpha1 / consistency_alpha2).
struct Bag {
    explicit Bag(const flow2d_host_params& params) : p(params)
    {
        bag.PushValuePtr("warp_levels_count", &p.warp_levels_count);
        bag.PushValuePtr("warp_scale_factor", &p.warp_scale_factor);
        bag.PushValuePtr("outer_iterations_count", &p.outer_iterations_count);
        bag.PushValuePtr("inner_iterations_count", &p.inner_iterations_count);
        bag.PushValuePtr("equation_alpha", &p.equation_alpha);
        bag.PushValuePtr("equation_smoothness", &p.equation_smoothness);
        bag.PushValuePtr("equation_data", &p.equation_data);
        bag.PushValuePtr("median_radius", &p.median_radius);
        bag.PushValuePtr("gaussian_sigma", &p.gaussian_sigma);
        bag.PushValuePtr("solver_algorithm", &p.solver_algorithm);
        bag.PushValuePtr("solver_sor_omega", &p.sor_omega);
    }
    Bag(const flow2d_host_params& params, float consistency_alpha1, float consistency_alpha2)
        : Bag(params)
    {
        alpha1 = consistency_alpha1;
        alpha2 = consistency_alpha2;
        bag.PushValuePtr("consistency_alpha1", &alpha1);
        bag.PushValuePtr("consistency_alpha2", &alpha2);
    }
    Bag(const Bag&) = delete;
    Bag& operator=(const Bag&) = delete;
    operator OperationParameters&() { return bag; }

    flow2d_host_params p;
    float alpha1 = 0.f, alpha2 = 0.f;
    OperationParameters bag;
};

// ... with the keys of a run from a prior flow: prior_reach, and prior_level when one is given (>= 0 from a caller; -1 = not given;
// anything below is passed on so that the entry refuses it)
struct PriorBag : Bag {
    PriorBag(const flow2d_host_params& params, float prior_reach, int prior_level) : Bag(params), reach(prior_reach), level(prior_level)
    {
        bag.PushValuePtr("prior_reach", &reach);
        if (level != -1) bag.PushValuePtr("prior_level", &level);
    }
    float reach;
    int level;
};

DevicePtr dp(void* q) { return static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(q)); }

// the `n` device addresses of `q` (none for a null array)
std::vector<DevicePtr> DevicePtrs(void* const* q, size_t n)
{
    std::vector<DevicePtr> out;
    for (size_t k = 0; q && k < n; ++k) out.push_back(dp(q[k]));
    return out;
}

// The images of a host-image entry on tight arrays (width * height floats per image, image k of an array at k * width * height).
class HostImages {
public:
    enum CopyBack { Always, AfterSuccess };

    explicit HostImages(const flow2d_host_flow* h) : width_(h->width), height_(h->height), n_(h->width * h->height) {}
    // `count` images holding copies of `src`: the first one (the others follow it in memory)
    Data2D* In(const float* src, size_t count = 1)
    {
        std::vector<Data2D>& images = Block(count);
        for (size_t k = 0; k < count; ++k) std::memcpy(images[k].DataPtr(), src + k * n_, n_ * sizeof(float));
        return images.data();
    }
    // `count` images that Finish() copies to `dst`: the first one, or null for a null `dst` (not wanted).  They are poisoned, and
    // those that are copied back Always show the poison to the caller after a run that was refused or failed.
    Data2D* Out(void* dst, CopyBack when, size_t count = 1)
    {
        if (!dst) return nullptr;
        std::vector<Data2D>& images = Block(count);
        for (size_t k = 0; k < count; ++k) {
            for (size_t i = 0; i < n_; ++i) images[k].DataPtr()[i] = -12345.f;
            outputs_.push_back({&images[k], static_cast<float*>(dst) + k * n_, when});
        }
        return images.data();
    }
    // After the run: the outputs into the caller's arrays, the device time into `total_ms` (optional); 0, or 2 when the run was
    // refused or an operator failed.
    int Finish(OpticalFlow2D& flow, float* total_ms = nullptr)
    {
        const bool ok = flow.LastRunSucceeded();
        for (const Output& o : outputs_)
            if (ok || o.when == Always) std::memcpy(o.dst, o.image->DataPtr(), n_ * sizeof(float));
        if (total_ms) *total_ms = flow.LastTotalMs();
        return ok ? 0 : 2;
    }

private:
    std::vector<Data2D>& Block(size_t count)
    {
        blocks_.emplace_back();
        for (size_t k = 0; k < count; ++k) blocks_.back().emplace_back(width_, height_);
        return blocks_.back();
    }
    struct Output {
        Data2D* image;
        float* dst;
        CopyBack when;
    };
    size_t width_, height_, n_;
    std::deque<std::vector<Data2D>> blocks_;  // (a deque: the blocks stay where they are)
    std::vector<Output> outputs_;
};

// the pointers to `count` images that follow each other
std::vector<Data2D*> Pointers(Data2D* images, size_t count)
{
    std::vector<Data2D*> out;
    for (size_t k = 0; k < count; ++k) out.push_back(images + k);
    return out;
}
}  // namespace

// Process-wide context on `device` (InitDeviceContext).  0 on success.
HOST_API int flow2d_host_init_device(int device) { return InitDeviceContext(device) ? 0 : 1; }
HOST_API void flow2d_host_adopt_context(flow2d_context* ctx) { AdoptDeviceContext(ctx); }
HOST_API flow2d_context* flow2d_host_context(void) { return CurrentDeviceContext(); }
HOST_API void flow2d_host_shutdown(void) { DestroyDeviceContext(); }

// constancy: enum class DataConstancy (0 Grey, 1 Gradient, 2 LogDerivatives, 3 GradientUntiled).  nullptr on failure.
// lone: OpticalFlow2D::lone (1: the object's pairs run alone on the device -- packed strip kernel for under-filled launches; 0: one
// worker among several)
HOST_API flow2d_host_flow* flow2d_host_flow_create(size_t width, size_t height, int constancy, int silent, int lone)
{
    flow2d_host_flow* h = new (std::nothrow) flow2d_host_flow();
    if (!h) return nullptr;
    h->flow.silent = silent != 0;
    h->flow.lone = lone != 0;
    DataSize3 size = {width, height, 1};
    if (!h->flow.Initialize(size, static_cast<DataConstancy>(constancy))) {
        delete h;
        return nullptr;
    }
    h->width = width;
    h->height = height;
    return h;
}

// ... initialised for lock-step groups of `group_size` pairs (OpticalFlow2D::group_size): what the entries that refuse groups refuse
HOST_API flow2d_host_flow* flow2d_host_flow_create_group(size_t width, size_t height, int constancy, size_t group_size)
{
    flow2d_host_flow* h = new (std::nothrow) flow2d_host_flow();
    if (!h) return nullptr;
    h->flow.silent = true;
    h->flow.group_size = group_size;
    DataSize3 size = {width, height, 1};
    if (!h->flow.Initialize(size, static_cast<DataConstancy>(constancy))) {
        delete h;
        return nullptr;
    }
    h->width = width;
    h->height = height;
    return h;
}

HOST_API void flow2d_host_flow_destroy(flow2d_host_flow* h)
{
    if (!h) return;
    h->flow.Destroy();
    delete h;
}

HOST_API size_t flow2d_host_flow_pitch(flow2d_host_flow* h) { return h ? h->flow.ContainerSize().pitch : 0; }

HOST_API size_t flow2d_host_max_warp_level(flow2d_host_flow* h, size_t width, size_t height, float scale)
{
    return h ? h->flow.GetMaxWarpLevel(width, height, scale) : 0;
}

// GetMaxWarpLevel needs no device (optical_flow_base_2d.cpp:36-59 is pure host arithmetic)
HOST_API size_t flow2d_host_max_warp_level_static(size_t width, size_t height, float scale)
{
    OpticalFlow2D flow;
    return flow.GetMaxWarpLevel(width, height, scale);
}

// OpticalFlow2D::ComputeFlow on tight host images (width*height floats each).  0 on success, 2 when the run
// delivered no flow.
HOST_API int flow2d_host_compute_flow(flow2d_host_flow* h, const float* frame_0, const float* frame_1, float* flow_u,
                                      float* flow_v, const flow2d_host_params* params, float* total_ms)
{
    if (!h || !frame_0 || !frame_1 || !flow_u || !flow_v || !params) return 1;
    // the outputs are poisoned so that an aborted run (missing key, bad parameter) is visible to the caller
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *u = im.Out(flow_u, im.Always), *v = im.Out(flow_v, im.Always);
    Bag bag(*params);
    h->flow.ComputeFlow(*f0, *f1, *u, *v, bag);
    return im.Finish(h->flow, total_ms);  // 2: the run was refused or an operator failed (outputs keep the poison)
}

// OpticalFlow2D::ComputeFlowDevice: frames and flow already in pitched device containers.  Queued on
// the context's stream, no synchronisation.  0 on success.
HOST_API int flow2d_host_compute_flow_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1,
                                             void* dev_flow_u, void* dev_flow_v, const flow2d_host_params* params,
                                             int timing_mode)
{
    if (!h || !params) return 1;
    Bag bag(*params);
    h->flow.timing_mode = timing_mode;
    return h->flow.ComputeFlowDevice(dp(dev_frame_0), dp(dev_frame_1), dp(dev_flow_u), dp(dev_flow_v), bag) ? 0 : 2;
}

// OpticalFlow2D::ComputeFlowSequenceDevice: frame_count device frames, frame_count - 1 flow plane pairs.
HOST_API int flow2d_host_compute_flow_sequence_device(flow2d_host_flow* h, void* const* dev_frames, size_t frame_count,
                                                      void* const* dev_flows_u, void* const* dev_flows_v,
                                                      const flow2d_host_params* params)
{
    if (!h || !params || !dev_frames || !dev_flows_u || !dev_flows_v || frame_count < 2) return 1;
    Bag bag(*params);
    h->flow.timing_mode = 0;
    const std::vector<DevicePtr> frames = DevicePtrs(dev_frames, frame_count), us = DevicePtrs(dev_flows_u, frame_count - 1),
                                 vs = DevicePtrs(dev_flows_v, frame_count - 1);
    return h->flow.ComputeFlowSequenceDevice(frames.data(), frame_count, us.data(), vs.data(), bag) ? 0 : 2;
}

// OpticalFlow2D::ComputeFlowBidirectional on tight host images (width*height floats each): forward and backward flow and both
// occlusion masks.  alpha1 / alpha2: the bag keys consistency_alpha1 / consistency_alpha2.  0 on success, 2 when the run
// delivered no flow.
HOST_API int flow2d_host_compute_flow_bidirectional(flow2d_host_flow* h, const float* frame_0, const float* frame_1,
                                                    float* flow_u, float* flow_v, float* back_u, float* back_v,
                                                    float* occlusion_0, float* occlusion_1, const flow2d_host_params* params,
                                                    float alpha1, float alpha2, float* total_ms)
{
    if (!h || !frame_0 || !frame_1 || !flow_u || !flow_v || !back_u || !back_v || !occlusion_0 || !occlusion_1 || !params)
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *out[6];
    float* dst[6] = {flow_u, flow_v, back_u, back_v, occlusion_0, occlusion_1};
    for (int i = 0; i < 6; ++i) out[i] = im.Out(dst[i], im.Always);
    Bag bag(*params, alpha1, alpha2);
    h->flow.ComputeFlowBidirectional(*f0, *f1, *out[0], *out[1], *out[2], *out[3], *out[4], *out[5], bag);
    return im.Finish(h->flow, total_ms);
}

// OpticalFlow2D::InterpolateFrames on tight host images (width*height floats each): the time_count frames of `times` between
// frame_0 and frame_1 into outputs (time_count * width * height floats, frame j at j * width * height).  use_masks = 0: without
// occlusion masks.  0 on success, 1 for a null argument, 2 when the run delivered no frames.
HOST_API int flow2d_host_interpolate_frames(flow2d_host_flow* h, const float* frame_0, const float* frame_1, const float* times,
                                            size_t time_count, float* outputs, const flow2d_host_params* params, int iterations,
                                            float max_residual, int use_masks, float* total_ms)
{
    if (!h || !frame_0 || !frame_1 || !times || !outputs || !params || time_count == 0) return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *out = im.Out(outputs, im.Always, time_count);
    Bag bag(*params);
    h->flow.InterpolateFrames(*f0, *f1, times, time_count, out, iterations, max_residual, use_masks != 0, bag);
    return im.Finish(h->flow, total_ms);
}

// OpticalFlow2D::InterpolateFramesDevice: frame_count device frames, (frame_count - 1) * time_count device output planes (pair k,
// time j at k * time_count + j).  Queued on the context's stream, no synchronisation.  0 on success.
HOST_API int flow2d_host_interpolate_frames_device(flow2d_host_flow* h, void* const* dev_frames, size_t frame_count,
                                                   const float* times, size_t time_count, void* const* dev_outputs,
                                                   const flow2d_host_params* params, int iterations, float max_residual,
                                                   int use_masks)
{
    if (!h || !params || !dev_frames || !dev_outputs || !times || frame_count < 2 || time_count == 0) return 1;
    Bag bag(*params);
    h->flow.timing_mode = 0;
    const std::vector<DevicePtr> frames = DevicePtrs(dev_frames, frame_count),
                                 outputs = DevicePtrs(dev_outputs, (frame_count - 1) * time_count);
    return h->flow.InterpolateFramesDevice(frames.data(), frame_count, times, time_count, outputs.data(), iterations, max_residual,
                                           use_masks != 0, bag)
               ? 0
               : 2;
}

// OpticalFlow2D::TrackPoints on tight host images: frames = frame_count * width * height floats (frame k at k * width * height);
// xs / ys get frame_count * capacity floats (table k at k * capacity), counts frame_count entries.  alpha1 / alpha2: the bag keys
// consistency_alpha1 / consistency_alpha2.  0 on success, 1 for a null argument, 2 when the run delivered no tracks.
HOST_API int flow2d_host_track_points(flow2d_host_flow* h, const float* frames, size_t frame_count, size_t spacing,
                                      float min_eigenvalue, int check_boundaries, float beta1, float beta2, float* xs, float* ys,
                                      size_t capacity, unsigned long long* counts, const flow2d_host_params* params, float alpha1,
                                      float alpha2, float* total_ms)
{
    if (!h || !frames || !xs || !ys || !counts || !params || frame_count < 2 || capacity == 0) return 1;
    HostImages im(h);
    const std::vector<Data2D*> fp = Pointers(im.In(frames, frame_count), frame_count);
    Bag bag(*params, alpha1, alpha2);
    h->flow.TrackPoints(fp.data(), frame_count, spacing, min_eigenvalue, check_boundaries != 0, beta1, beta2, xs, ys, capacity,
                        counts, bag);
    return im.Finish(h->flow, total_ms);
}

// OpticalFlow2D::TrackPointsDevice: frame_count device frames and frame_count device tables of `capacity` floats per
// coordinate; counts (host) gets frame_count entries.  Synchronises once at the end.  0 on success.
HOST_API int flow2d_host_track_points_device(flow2d_host_flow* h, void* const* dev_frames, size_t frame_count, size_t spacing,
                                             float min_eigenvalue, int check_boundaries, float beta1, float beta2,
                                             void* const* dev_xs, void* const* dev_ys, size_t capacity,
                                             unsigned long long* counts, const flow2d_host_params* params, float alpha1,
                                             float alpha2)
{
    if (!h || !params || !dev_frames || !dev_xs || !dev_ys || !counts || frame_count < 2 || capacity == 0) return 1;
    Bag bag(*params, alpha1, alpha2);
    h->flow.timing_mode = 0;
    const std::vector<DevicePtr> frames = DevicePtrs(dev_frames, frame_count), xs = DevicePtrs(dev_xs, frame_count),
                                 ys = DevicePtrs(dev_ys, frame_count);
    return h->flow.TrackPointsDevice(frames.data(), frame_count, spacing, min_eigenvalue, check_boundaries != 0, beta1, beta2,
                                     xs.data(), ys.data(), capacity, counts, bag)
               ? 0
               : 2;
}

// OpticalFlow2D::DenoiseArgsOk: 1 when frame_count, radius and range_sigma are what DenoiseSequence* accept.  Needs no device.
HOST_API int flow2d_host_denoise_args_ok(size_t frame_count, size_t radius, float range_sigma)
{
    return OpticalFlow2D::DenoiseArgsOk(frame_count, radius, range_sigma) ? 1 : 0;
}

// OpticalFlow2D::DenoiseSequence on tight host images: frames = frame_count * width * height floats (frame k at k * width *
// height); outputs, and weight_sums when not NULL, get the same layout.  0 on success, 1 for a null or refused argument, 2 when the
// run delivered no frames.
HOST_API int flow2d_host_denoise_sequence(flow2d_host_flow* h, const float* frames, size_t frame_count, size_t radius,
                                          float range_sigma, int use_masks, float* outputs, float* weight_sums,
                                          const flow2d_host_params* params, float* total_ms)
{
    if (!OpticalFlow2D::DenoiseArgsOk(frame_count, radius, range_sigma) || !h || !frames || !outputs || !params) return 1;
    HostImages im(h);
    const std::vector<Data2D*> fp = Pointers(im.In(frames, frame_count), frame_count);
    Data2D *out = im.Out(outputs, im.Always, frame_count), *sums = im.Out(weight_sums, im.AfterSuccess, frame_count);
    Bag bag(*params);
    h->flow.DenoiseSequence(fp.data(), frame_count, radius, range_sigma, use_masks != 0, out, sums, bag);
    return im.Finish(h->flow, total_ms);
}

// OpticalFlow2D::DenoiseSequenceDevice: frame_count device frames and output planes, weight-sum planes optional (NULL: none).
// Queued on the context's stream, no synchronisation.  0 on success, 1 for a null or refused argument.
HOST_API int flow2d_host_denoise_sequence_device(flow2d_host_flow* h, void* const* dev_frames, size_t frame_count, size_t radius,
                                                 float range_sigma, int use_masks, void* const* dev_outputs,
                                                 void* const* dev_weight_sums, const flow2d_host_params* params)
{
    if (!OpticalFlow2D::DenoiseArgsOk(frame_count, radius, range_sigma) || !h || !params || !dev_frames || !dev_outputs) return 1;
    Bag bag(*params);
    h->flow.timing_mode = 0;
    const std::vector<DevicePtr> frames = DevicePtrs(dev_frames, frame_count), outputs = DevicePtrs(dev_outputs, frame_count),
                                 sums = DevicePtrs(dev_weight_sums, frame_count);
    return h->flow.DenoiseSequenceDevice(frames.data(), frame_count, radius, range_sigma, use_masks != 0, outputs.data(),
                                         dev_weight_sums ? sums.data() : nullptr, bag)
               ? 0
               : 2;
}

// OpticalFlow2D::GlobalMotionArgsOk: 1 when model, sigma and iterations are what the global-motion entries accept.  Needs no device.
HOST_API int flow2d_host_global_motion_args_ok(int model, double sigma, int iterations)
{
    return OpticalFlow2D::GlobalMotionArgsOk(model, sigma, iterations) ? 1 : 0;
}

// OpticalFlow2D::ComposeGlobalMotion: `second` after `first` into `out`.  Needs no device.  0 on success, 1 for a null argument.
HOST_API int flow2d_host_compose_global_motion(const flow2d_global_motion* first, const flow2d_global_motion* second,
                                               flow2d_global_motion* out)
{
    if (!first || !second || !out) return 1;
    *out = OpticalFlow2D::ComposeGlobalMotion(*first, *second);
    return 0;
}

// OpticalFlow2D::EstimateGlobalMotion on tight host images (width*height floats each): the record of the pair into `motion`;
// flow_u / flow_v and residual_u / residual_v (each pair optional) get the flow and the residual flow.  0 on success, 1 for a
// null or refused argument, 2 when the run delivered nothing.
HOST_API int flow2d_host_estimate_global_motion(flow2d_host_flow* h, const float* frame_0, const float* frame_1, int model,
                                                double sigma, int iterations, int use_masks, flow2d_global_motion* motion,
                                                const flow2d_host_params* params, float* flow_u, float* flow_v,
                                                float* residual_u, float* residual_v, float* total_ms)
{
    if (!OpticalFlow2D::GlobalMotionArgsOk(model, sigma, iterations) || !h || !frame_0 || !frame_1 || !motion || !params ||
        (flow_u == nullptr) != (flow_v == nullptr) || (residual_u == nullptr) != (residual_v == nullptr))
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *out[4];
    float* dst[4] = {flow_u, flow_v, residual_u, residual_v};
    for (int i = 0; i < 4; ++i) out[i] = im.Out(dst[i], im.AfterSuccess);
    Bag bag(*params);
    h->flow.EstimateGlobalMotion(*f0, *f1, model, sigma, iterations, use_masks != 0, motion, bag, out[0], out[1], out[2], out[3]);
    return im.Finish(h->flow, total_ms);
}

// OpticalFlow2D::EstimateGlobalMotionDevice: two device frames, the record into `motion` (host); the optional device planes
// get the flow and the residual flow.  Synchronises.  0 on success, 1 for a null or refused argument.
HOST_API int flow2d_host_estimate_global_motion_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, int model,
                                                       double sigma, int iterations, int use_masks, flow2d_global_motion* motion,
                                                       const flow2d_host_params* params, void* dev_flow_u, void* dev_flow_v,
                                                       void* dev_residual_u, void* dev_residual_v)
{
    if (!OpticalFlow2D::GlobalMotionArgsOk(model, sigma, iterations) || !h || !dev_frame_0 || !dev_frame_1 || !motion || !params)
        return 1;
    Bag bag(*params);
    h->flow.timing_mode = 0;
    return h->flow.EstimateGlobalMotionDevice(dp(dev_frame_0), dp(dev_frame_1), model, sigma, iterations, use_masks != 0, motion, bag,
                                              dp(dev_flow_u), dp(dev_flow_v), dp(dev_residual_u), dp(dev_residual_v))
               ? 0
               : 2;
}

// OpticalFlow2D::SegmentMotionArgsOk: 1 when threshold, join and min_area are what flow2d_segment_motion_2d accepts.  Needs no device.
HOST_API int flow2d_host_segment_motion_args_ok(float threshold, float join, unsigned min_area)
{
    return OpticalFlow2D::SegmentMotionArgsOk(threshold, join, min_area) ? 1 : 0;
}

// How many records flow2d_host_segment_motion* write into `regions` (OpticalFlow2D::kSegmentMaxRegions).
HOST_API size_t flow2d_host_segment_max_regions() { return OpticalFlow2D::kSegmentMaxRegions; }

// OpticalFlow2D::SegmentMotion on tight host images: the record, the summary and the region table (regions: optional,
// flow2d_host_segment_max_regions() records); labels (width*height ints) and residual_u / residual_v (optional) get the planes.
// 0 on success, 1 for a null or refused argument, 2 when the run delivered nothing.
HOST_API int flow2d_host_segment_motion(flow2d_host_flow* h, const float* frame_0, const float* frame_1, int model, double sigma,
                                        int iterations, int use_masks, float threshold, float join, unsigned min_area,
                                        flow2d_global_motion* motion, flow2d_segment_summary* summary, flow2d_motion_region* regions,
                                        const flow2d_host_params* params, int* labels, float* residual_u, float* residual_v)
{
    if (!OpticalFlow2D::GlobalMotionArgsOk(model, sigma, iterations) || !OpticalFlow2D::SegmentMotionArgsOk(threshold, join, min_area) ||
        !h || !frame_0 || !frame_1 || !motion || !summary || !params || (residual_u == nullptr) != (residual_v == nullptr))
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *out[3];
    void* dst[3] = {labels, residual_u, residual_v};
    for (int i = 0; i < 3; ++i) out[i] = im.Out(dst[i], im.AfterSuccess);
    Bag bag(*params);
    h->flow.SegmentMotion(*f0, *f1, model, sigma, iterations, use_masks != 0, threshold, join, min_area, motion, summary, regions, bag,
                          out[0], out[1], out[2]);
    return im.Finish(h->flow);
}

// OpticalFlow2D::SegmentMotionDevice: two device frames; the optional device planes get the labels and the residual flow.
// Synchronises.  0 on success, 1 for a null or refused argument.
HOST_API int flow2d_host_segment_motion_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, int model, double sigma,
                                               int iterations, int use_masks, float threshold, float join, unsigned min_area,
                                               flow2d_global_motion* motion, flow2d_segment_summary* summary,
                                               flow2d_motion_region* regions, const flow2d_host_params* params, void* dev_labels,
                                               void* dev_residual_u, void* dev_residual_v)
{
    if (!OpticalFlow2D::GlobalMotionArgsOk(model, sigma, iterations) || !OpticalFlow2D::SegmentMotionArgsOk(threshold, join, min_area) ||
        !h || !dev_frame_0 || !dev_frame_1 || !motion || !summary || !params)
        return 1;
    Bag bag(*params);
    h->flow.timing_mode = 0;
    return h->flow.SegmentMotionDevice(dp(dev_frame_0), dp(dev_frame_1), model, sigma, iterations, use_masks != 0, threshold, join,
                                       min_area, motion, summary, regions, bag, dp(dev_labels), dp(dev_residual_u), dp(dev_residual_v))
               ? 0
               : 2;
}

// OpticalFlow2D::DeformationArgsOk: 1 when measure and smoothing_sigma are what AnalyseDeformation accepts.  Needs no device.
HOST_API int flow2d_host_deformation_args_ok(int measure, float smoothing_sigma)
{
    return OpticalFlow2D::DeformationArgsOk(measure, smoothing_sigma) ? 1 : 0;
}

// OpticalFlow2D::AnalyseDeformation on tight host images: planes = nine pointers in the order of flow2d_deformation_planes (each
// may be null, as may the array), width*height floats each; stats (optional) gets the record, flow_u / flow_v (optional) the flow
// that was analysed, mask (optional, use_masks only) the occlusion mask.  0 on success, 1 for a null or refused argument, 2 when
// the run delivered nothing.
HOST_API int flow2d_host_analyse_deformation(flow2d_host_flow* h, const float* frame_0, const float* frame_1, int measure,
                                             float smoothing_sigma, int use_masks, float* const* planes,
                                             flow2d_deformation_stats* stats, const flow2d_host_params* params, float* flow_u,
                                             float* flow_v, float* mask)
{
    if (!OpticalFlow2D::DeformationArgsOk(measure, smoothing_sigma) || !h || !frame_0 || !frame_1 || !params ||
        (flow_u == nullptr) != (flow_v == nullptr) || (mask && !use_masks))
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *out[12];
    float* dst[12] = {flow_u, flow_v, mask};
    for (int k = 0; k < 9; ++k) dst[3 + k] = planes ? planes[k] : nullptr;
    for (int i = 0; i < 12; ++i) out[i] = im.Out(dst[i], im.AfterSuccess);
    Bag bag(*params);
    h->flow.AnalyseDeformation(*f0, *f1, measure, smoothing_sigma, use_masks != 0, out + 3, stats, bag, out[0], out[1], out[2]);
    return im.Finish(h->flow);
}

// OpticalFlow2D::AnalyseDeformationDevice: two device frames; dev_planes = nine device planes (each may be null, as may the
// array); the optional device planes get the analysed flow and the mask.  Synchronises.  0 on success, 1 for a null or refused
// argument.
HOST_API int flow2d_host_analyse_deformation_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, int measure,
                                                    float smoothing_sigma, int use_masks, void* const* dev_planes,
                                                    flow2d_deformation_stats* stats, const flow2d_host_params* params,
                                                    void* dev_flow_u, void* dev_flow_v, void* dev_mask)
{
    if (!OpticalFlow2D::DeformationArgsOk(measure, smoothing_sigma) || !h || !dev_frame_0 || !dev_frame_1 || !params) return 1;
    Bag bag(*params);
    h->flow.timing_mode = 0;
    DevicePtr planes[9];
    for (int k = 0; k < 9; ++k) planes[k] = dev_planes ? dp(dev_planes[k]) : 0;
    return h->flow.AnalyseDeformationDevice(dp(dev_frame_0), dp(dev_frame_1), measure, smoothing_sigma, use_masks != 0, planes, stats,
                                            bag, dp(dev_flow_u), dp(dev_flow_v), dp(dev_mask))
               ? 0
               : 2;
}

// OpticalFlow2D::RefineArgsOk: 1 when the arguments are what RefineFlow accepts.  Needs no device.
HOST_API int flow2d_host_refine_args_ok(int radius, float sigma_guide, float sigma_space, int iterations)
{
    return OpticalFlow2D::RefineArgsOk(radius, sigma_guide, sigma_space, iterations) ? 1 : 0;
}

// OpticalFlow2D::RefineFlow on tight host images: refined_u / refined_v get the refined flow, record (optional) the counts of the
// last pass, flow_u / flow_v (optional) the flow before the refinement, mask (optional, use_masks only) the occlusion mask.  0 on
// success, 1 for a null or refused argument, 2 when the run delivered nothing.
HOST_API int flow2d_host_refine_flow(flow2d_host_flow* h, const float* frame_0, const float* frame_1, int radius, float sigma_guide,
                                     float sigma_space, int iterations, int use_masks, float* refined_u, float* refined_v,
                                     flow2d_refine_record* record, const flow2d_host_params* params, float* flow_u, float* flow_v,
                                     float* mask)
{
    if (!OpticalFlow2D::RefineArgsOk(radius, sigma_guide, sigma_space, iterations) || !h || !frame_0 || !frame_1 || !refined_u ||
        !refined_v || !params || (flow_u == nullptr) != (flow_v == nullptr) || (mask && !use_masks))
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *out[5];
    float* dst[5] = {refined_u, refined_v, flow_u, flow_v, mask};
    for (int i = 0; i < 5; ++i) out[i] = im.Out(dst[i], im.AfterSuccess);
    Bag bag(*params);
    h->flow.RefineFlow(*f0, *f1, radius, sigma_guide, sigma_space, iterations, use_masks != 0, *out[0], *out[1], record, bag, out[2],
                       out[3], out[4]);
    return im.Finish(h->flow);
}

// OpticalFlow2D::RefineFlowDevice: device planes; with flow_given the flow planes (and the optional mask) are the flow to refine
// and dev_frame_1 may be null.  Synchronises.  0 on success, 1 for a null or refused argument, 2 when the run failed.
HOST_API int flow2d_host_refine_flow_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, int radius, float sigma_guide,
                                            float sigma_space, int iterations, int use_masks, void* dev_refined_u,
                                            void* dev_refined_v, flow2d_refine_record* record, const flow2d_host_params* params,
                                            void* dev_flow_u, void* dev_flow_v, void* dev_mask, int flow_given)
{
    if (!OpticalFlow2D::RefineArgsOk(radius, sigma_guide, sigma_space, iterations) || !h || !dev_frame_0 || !dev_refined_u ||
        !dev_refined_v || !params)
        return 1;
    Bag bag(*params);
    h->flow.timing_mode = 0;
    return h->flow.RefineFlowDevice(dp(dev_frame_0), dp(dev_frame_1), radius, sigma_guide, sigma_space, iterations, use_masks != 0,
                                    dp(dev_refined_u), dp(dev_refined_v), record, bag, dp(dev_flow_u), dp(dev_flow_v), dp(dev_mask),
                                    flow_given != 0)
               ? 0
               : 2;
}

// OpticalFlow2D::CorrelationArgsOk: 1 when the arguments are what Correlate* accepts for a width x height frame.  Needs no device.
HOST_API int flow2d_host_correlation_args_ok(size_t width, size_t height, float lo, float scale, int radius, int range, int spacing,
                                             float min_score)
{
    return OpticalFlow2D::CorrelationArgsOk(width, height, lo, scale, radius, range, spacing, min_score) ? 1 : 0;
}

// OpticalFlow2D::Correlate on tight host images: node_u / node_v / node_score (optional) get nw * nh floats each (the grid of
// flow2d_correlation_grid), record (optional) the counts, flow_u / flow_v (optional, both or neither) the field on the frame's
// grid, lo_scale (optional) the two numbers of OpticalFlow2D::CorrelationRange the frames were quantised with.  0 on success, 1 for
// a null or refused argument, 2 when the run delivered nothing.
HOST_API int flow2d_host_correlate(flow2d_host_flow* h, const float* frame_0, const float* frame_1, int radius, int range, int spacing,
                                   float min_score, float* node_u, float* node_v, float* node_score, flow2d_correlation_record* record,
                                   float* flow_u, float* flow_v, float* lo_scale)
{
    size_t nw = 0, nh = 0;
    if (!h || !frame_0 || !frame_1 || !node_u || !node_v || (flow_u == nullptr) != (flow_v == nullptr) ||
        flow2d_correlation_grid(h->width, h->height, radius, spacing, &nw, &nh) != FLOW2D_OK)
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1);
    Data2D *fu = im.Out(flow_u, im.AfterSuccess), *fv = im.Out(flow_v, im.AfterSuccess);
    float lo = 0.f, scale = 1.f;
    OpticalFlow2D::CorrelationRange(*f0, *f1, lo, scale);
    if (!OpticalFlow2D::CorrelationArgsOk(h->width, h->height, lo, scale, radius, range, spacing, min_score)) return 1;
    Data2D nodes[3] = {Data2D(nw, nh), Data2D(nw, nh), Data2D(nw, nh)};
    h->flow.Correlate(*f0, *f1, radius, range, spacing, min_score, nodes[0], nodes[1], node_score ? &nodes[2] : nullptr, record, fu, fv);
    const int rc = im.Finish(h->flow);
    if (rc) return rc;
    float* dst[3] = {node_u, node_v, node_score};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) std::memcpy(dst[k], nodes[k].DataPtr(), nw * nh * sizeof(float));
    if (lo_scale) {
        lo_scale[0] = lo;
        lo_scale[1] = scale;
    }
    return 0;
}

// OpticalFlow2D::CorrelateDevice: device planes of the container's size (the node planes optional).  Synchronises.  0 on success, 1
// for a null or refused argument, 2 when the run failed.
HOST_API int flow2d_host_correlate_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, float lo, float scale, int radius,
                                          int range, int spacing, float min_score, void* dev_node_u, void* dev_node_v,
                                          void* dev_node_score, flow2d_correlation_record* record, void* dev_flow_u, void* dev_flow_v)
{
    if (!h || !dev_frame_0 || !dev_frame_1 || (dev_flow_u == nullptr) != (dev_flow_v == nullptr) ||
        !OpticalFlow2D::CorrelationArgsOk(h->width, h->height, lo, scale, radius, range, spacing, min_score))
        return 1;
    h->flow.timing_mode = 0;
    return h->flow.CorrelateDevice(dp(dev_frame_0), dp(dev_frame_1), lo, scale, radius, range, spacing, min_score, dp(dev_node_u),
                                   dp(dev_node_v), dp(dev_node_score), record, dp(dev_flow_u), dp(dev_flow_v))
               ? 0
               : 2;
}

// ---- multi-pass window correlation -----------------------------------------------------------------------------------------------
// passes: three ints per pass (radius, range, spacing).
static std::vector<OpticalFlow2D::CorrelationPass> correlation_passes(const int* passes, int count)
{
    std::vector<OpticalFlow2D::CorrelationPass> out;
    for (int k = 0; passes && k < count; ++k) out.push_back({passes[3 * k], passes[3 * k + 1], passes[3 * k + 2]});
    return out;
}

static OpticalFlow2D::ValidationOptions validation_options(float threshold, float epsilon, int min_neighbours, int replace, int validate_last)
{
    OpticalFlow2D::ValidationOptions v;
    v.threshold = threshold;
    v.epsilon = epsilon;
    v.min_neighbours = min_neighbours;
    v.replace = replace != 0;
    v.validate_last = validate_last != 0;
    return v;
}

// OpticalFlow2D::CorrelationPassesOk: 1 when the schedule and the validation options are what CorrelateMultiPass* accepts for a
// width x height frame.  Needs no device.
HOST_API int flow2d_host_correlation_passes_ok(size_t width, size_t height, float lo, float scale, const int* passes, int count,
                                               float min_score, float threshold, float epsilon, int min_neighbours)
{
    const auto list = correlation_passes(passes, count);
    return count >= 0 && OpticalFlow2D::CorrelationPassesOk(width, height, lo, scale, list.data(), list.size(), min_score,
                                                            validation_options(threshold, epsilon, min_neighbours, 1, 1))
               ? 1
               : 0;
}

// OpticalFlow2D::CorrelateMultiPassDevice: device planes of the container's size (predictor, node planes, score and flow optional);
// reports (optional): one OpticalFlow2D::CorrelationPassReport per pass.  Synchronises.  0 on success, 1 for a null or refused
// argument, 2 when the run failed.
HOST_API int flow2d_host_correlate_multipass_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, float lo, float scale,
                                                    const int* passes, int count, float min_score, float threshold, float epsilon,
                                                    int min_neighbours, int replace, int validate_last, void* dev_predictor_u,
                                                    void* dev_predictor_v, void* dev_node_u, void* dev_node_v, void* dev_node_score,
                                                    OpticalFlow2D::CorrelationPassReport* reports, void* dev_flow_u, void* dev_flow_v)
{
    const auto list = correlation_passes(passes, count);
    const auto validation = validation_options(threshold, epsilon, min_neighbours, replace, validate_last);
    if (!h || !dev_frame_0 || !dev_frame_1 || count < 0 || (dev_flow_u == nullptr) != (dev_flow_v == nullptr) ||
        (dev_predictor_u == nullptr) != (dev_predictor_v == nullptr) || (dev_node_u == nullptr) != (dev_node_v == nullptr) ||
        !OpticalFlow2D::CorrelationPassesOk(h->width, h->height, lo, scale, list.data(), list.size(), min_score, validation))
        return 1;
    h->flow.timing_mode = 0;
    return h->flow.CorrelateMultiPassDevice(dp(dev_frame_0), dp(dev_frame_1), lo, scale, list.data(), list.size(), min_score, validation,
                                            dp(dev_predictor_u), dp(dev_predictor_v), dp(dev_node_u), dp(dev_node_v), dp(dev_node_score),
                                            reports, dp(dev_flow_u), dp(dev_flow_v))
               ? 0
               : 2;
}

// OpticalFlow2D::CorrelateMultiPass on tight host images: node_u / node_v / node_score (optional) get the last pass's nw * nh
// floats each, flow_u / flow_v (optional, both or neither) its field on the frame's grid, predictor_u / predictor_v (optional,
// both or neither) are the initial predictor, lo_scale (optional) the two numbers of CorrelationRange.
HOST_API int flow2d_host_correlate_multipass(flow2d_host_flow* h, const float* frame_0, const float* frame_1, const int* passes, int count,
                                             float min_score, float threshold, float epsilon, int min_neighbours, int replace,
                                             int validate_last, const float* predictor_u, const float* predictor_v, float* node_u,
                                             float* node_v, float* node_score, OpticalFlow2D::CorrelationPassReport* reports,
                                             float* flow_u, float* flow_v, float* lo_scale)
{
    const auto list = correlation_passes(passes, count);
    const auto validation = validation_options(threshold, epsilon, min_neighbours, replace, validate_last);
    if (!h || !frame_0 || !frame_1 || !node_u || !node_v || count < 0 || (flow_u == nullptr) != (flow_v == nullptr) ||
        (predictor_u == nullptr) != (predictor_v == nullptr))
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1);
    Data2D *pu = predictor_u ? im.In(predictor_u) : nullptr, *pv = predictor_v ? im.In(predictor_v) : nullptr;
    Data2D *fu = im.Out(flow_u, im.AfterSuccess), *fv = im.Out(flow_v, im.AfterSuccess);
    float lo = 0.f, scale = 1.f;
    OpticalFlow2D::CorrelationRange(*f0, *f1, lo, scale);
    if (!OpticalFlow2D::CorrelationPassesOk(h->width, h->height, lo, scale, list.data(), list.size(), min_score, validation)) return 1;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(h->width, h->height, list.back().radius, list.back().spacing, &nw, &nh);
    Data2D nodes[3] = {Data2D(nw, nh), Data2D(nw, nh), Data2D(nw, nh)};
    h->flow.CorrelateMultiPass(*f0, *f1, list.data(), list.size(), min_score, validation, nodes[0], nodes[1],
                               node_score ? &nodes[2] : nullptr, reports, fu, fv, pu, pv);
    const int rc = im.Finish(h->flow);
    if (rc) return rc;
    float* dst[3] = {node_u, node_v, node_score};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) std::memcpy(dst[k], nodes[k].DataPtr(), nw * nh * sizeof(float));
    if (lo_scale) {
        lo_scale[0] = lo;
        lo_scale[1] = scale;
    }
    return 0;
}

// OpticalFlow2D::CorrelationPassesOk with ValidationOptions::min_pixels: 1 when the schedule takes that min_pixels (0: the default
// per pass) beside everything flow2d_host_correlation_passes_ok checks.  Needs no device.
HOST_API int flow2d_host_correlation_passes_masked_ok(size_t width, size_t height, float lo, float scale, const int* passes, int count,
                                                      float min_score, float threshold, float epsilon, int min_neighbours, int min_pixels)
{
    const auto list = correlation_passes(passes, count);
    auto validation = validation_options(threshold, epsilon, min_neighbours, 1, 1);
    validation.min_pixels = min_pixels;
    return count >= 0 && OpticalFlow2D::CorrelationPassesOk(width, height, lo, scale, list.data(), list.size(), min_score, validation) ? 1 : 0;
}

// flow2d_host_correlate_multipass_device on a region of interest (ValidationOptions::mask, min_pixels): dev_mask is a device plane
// of the container's size, null for none -- the call is then that entry's --, min_pixels 0 the default per pass.  The masked
// counts are the seventh words of the reports' records.
HOST_API int flow2d_host_correlate_multipass_masked_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, float lo, float scale,
                                                           const int* passes, int count, float min_score, float threshold, float epsilon,
                                                           int min_neighbours, int replace, int validate_last, void* dev_mask,
                                                           int min_pixels, void* dev_predictor_u, void* dev_predictor_v, void* dev_node_u,
                                                           void* dev_node_v, void* dev_node_score,
                                                           OpticalFlow2D::CorrelationPassReport* reports, void* dev_flow_u, void* dev_flow_v)
{
    const auto list = correlation_passes(passes, count);
    auto validation = validation_options(threshold, epsilon, min_neighbours, replace, validate_last);
    validation.mask = dp(dev_mask);
    validation.min_pixels = min_pixels;
    if (!h || !dev_frame_0 || !dev_frame_1 || count < 0 || (dev_flow_u == nullptr) != (dev_flow_v == nullptr) ||
        (dev_predictor_u == nullptr) != (dev_predictor_v == nullptr) || (dev_node_u == nullptr) != (dev_node_v == nullptr) ||
        !OpticalFlow2D::CorrelationPassesOk(h->width, h->height, lo, scale, list.data(), list.size(), min_score, validation))
        return 1;
    h->flow.timing_mode = 0;
    return h->flow.CorrelateMultiPassDevice(dp(dev_frame_0), dp(dev_frame_1), lo, scale, list.data(), list.size(), min_score, validation,
                                            dp(dev_predictor_u), dp(dev_predictor_v), dp(dev_node_u), dp(dev_node_v), dp(dev_node_score),
                                            reports, dp(dev_flow_u), dp(dev_flow_v))
               ? 0
               : 2;
}

// flow2d_host_correlate_multipass on a region of interest: mask is a tight host image of the frames' size (null: none), which the
// object uploads once; the rest as there and above.
HOST_API int flow2d_host_correlate_multipass_masked(flow2d_host_flow* h, const float* frame_0, const float* frame_1, const int* passes,
                                                    int count, float min_score, float threshold, float epsilon, int min_neighbours,
                                                    int replace, int validate_last, const float* mask, int min_pixels,
                                                    const float* predictor_u, const float* predictor_v, float* node_u, float* node_v,
                                                    float* node_score, OpticalFlow2D::CorrelationPassReport* reports, float* flow_u,
                                                    float* flow_v, float* lo_scale)
{
    const auto list = correlation_passes(passes, count);
    auto validation = validation_options(threshold, epsilon, min_neighbours, replace, validate_last);
    validation.min_pixels = min_pixels;
    if (!h || !frame_0 || !frame_1 || !node_u || !node_v || count < 0 || (flow_u == nullptr) != (flow_v == nullptr) ||
        (predictor_u == nullptr) != (predictor_v == nullptr))
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1);
    Data2D *pu = predictor_u ? im.In(predictor_u) : nullptr, *pv = predictor_v ? im.In(predictor_v) : nullptr;
    Data2D *fu = im.Out(flow_u, im.AfterSuccess), *fv = im.Out(flow_v, im.AfterSuccess);
    Data2D* region = mask ? im.In(mask) : nullptr;
    float lo = 0.f, scale = 1.f;
    OpticalFlow2D::CorrelationRange(*f0, *f1, lo, scale);
    if (!OpticalFlow2D::CorrelationPassesOk(h->width, h->height, lo, scale, list.data(), list.size(), min_score, validation)) return 1;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(h->width, h->height, list.back().radius, list.back().spacing, &nw, &nh);
    Data2D nodes[3] = {Data2D(nw, nh), Data2D(nw, nh), Data2D(nw, nh)};
    h->flow.CorrelateMultiPass(*f0, *f1, list.data(), list.size(), min_score, validation, nodes[0], nodes[1],
                               node_score ? &nodes[2] : nullptr, reports, fu, fv, pu, pv, region);
    const int rc = im.Finish(h->flow);
    if (rc) return rc;
    float* dst[3] = {node_u, node_v, node_score};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) std::memcpy(dst[k], nodes[k].DataPtr(), nw * nh * sizeof(float));
    if (lo_scale) {
        lo_scale[0] = lo;
        lo_scale[1] = scale;
    }
    return 0;
}

// ---- subset refinement of correlation nodes -----------------------------------------------------------------------------------
// Every entry that refines takes OpticalFlow2D::SubsetOptions as one record (null: refused) and its outputs as the fourteen slots
// of OpticalFlow2D::SubsetPlanes -- u, v, ux, uy, vx, vy, score, state, then uxx, uxy, uyy, vxx, vxy, vyy --, per step in the
// sequence forms.  The six curvatures go with order 2: at order 1 a slot of theirs that is set is refused, and the host-image
// forms allocate and copy the eight images only.  A new field of SubsetOptions is a new field of the record, not a new entry --
// with one exception, SubsetOptions::interpolation: the record's size and field list are what callers built against the library
// hold (40 bytes, nine fields), so the choice travels beside it, kept in the object by flow2d_host_set_subset_interpolation and
// copied into the SubsetOptions every entry below builds.
struct flow2d_host_subset_options {
    int radius, iterations;
    float epsilon, max_shift, max_gradient;
    int order;  // 1 or 2
    float max_curvature;
    int min_pixels;    // 0: the default of the radius
    const void* mask;  // null: none.  *_device entries: a device plane of the container's size; host-image entries: a tight host
                       // image of the frames' size; flow2d_host_subset_options_ok: any non-null value means "with a mask"
};

namespace {
constexpr int kSubsetSlots = 14;

// (the mask of a host-image entry stays its host address here: the mark SubsetOptionsOk looks at -- CorrelateSubset* take the
// image itself and do not look at the field)
OpticalFlow2D::SubsetOptions subset_options(const flow2d_host_subset_options& record, const flow2d_host_flow* h = nullptr)
{
    OpticalFlow2D::SubsetOptions o;
    if (h) o.interpolation = h->subset_interpolation;
    o.radius = record.radius;
    o.iterations = record.iterations;
    o.epsilon = record.epsilon;
    o.max_shift = record.max_shift;
    o.max_gradient = record.max_gradient;
    o.order = record.order;
    o.max_curvature = record.max_curvature;
    o.mask = dp(const_cast<void*>(record.mask));
    o.min_pixels = record.min_pixels;
    o.mask_search = h && h->subset_mask_search;
    return o;
}

// fourteen device planes, each of which may be null, as may the array
OpticalFlow2D::SubsetPlanes subset_planes(void* const* p)
{
    OpticalFlow2D::SubsetPlanes o;
    if (p)
        o = {dp(p[0]), dp(p[1]), dp(p[2]), dp(p[3]),  dp(p[4]),  dp(p[5]),  dp(p[6]),
             dp(p[7]), dp(p[8]), dp(p[9]), dp(p[10]), dp(p[11]), dp(p[12]), dp(p[13])};
    return o;
}

// the node images of a step: what the host-image forms of OpticalFlow2D take per step
int node_images(const OpticalFlow2D::SubsetOptions& subset) { return subset.order == 2 ? kSubsetSlots : 8; }

// OpticalFlow2D::SubsetOptionsOk, and no curvature slot of the `steps` sets of fourteen (null: none) set at order 1
template <typename Pointer>
bool subset_accepted(const OpticalFlow2D::SubsetOptions& subset, Pointer const* slots, size_t steps = 1)
{
    if (!OpticalFlow2D::SubsetOptionsOk(subset)) return false;
    for (size_t k = 0; slots && subset.order != 2 && k < steps; ++k)
        for (int c = 8; c < kSubsetSlots; ++c)
            if (slots[kSubsetSlots * k + c]) return false;
    return true;
}
}  // namespace

// OpticalFlow2D::SubsetOptionsOk: 1 when the options are what RefineNodes* / CorrelateSubset* accept.  Needs no device.
HOST_API int flow2d_host_subset_options_ok(const flow2d_host_subset_options* options)
{
    return options && OpticalFlow2D::SubsetOptionsOk(subset_options(*options)) ? 1 : 0;
}

// Whether `kind` is a value of OpticalFlow2D::SubsetOptions::Interpolation.  Needs no device.
HOST_API int flow2d_host_subset_interpolation_ok(int kind)
{
    return kind == OpticalFlow2D::SubsetOptions::CatmullRom || kind == OpticalFlow2D::SubsetOptions::BSpline ? 1 : 0;
}

// OpticalFlow2D::SubsetOptions::interpolation of every later call of this object that refines: 0 Catmull-Rom (what a new object
// has), 1 cubic B-spline.  0 on success, 1 for a null object or an unknown kind, which changes nothing.
HOST_API int flow2d_host_set_subset_interpolation(flow2d_host_flow* h, int kind)
{
    if (!h || !flow2d_host_subset_interpolation_ok(kind)) return 1;
    h->subset_interpolation = kind;
    return 0;
}

// OpticalFlow2D::SubsetOptions::mask_search of every later call of this object that runs the passes of a pair in front of a
// refinement with a mask (it travels beside the 40-byte options record, like the interpolation): 0 off (what a new object has),
// 1 on -- every entry below then refuses options without a mask, as SubsetOptionsOk does.  0 on success, 1 for a null object or
// another value, which changes nothing.
HOST_API int flow2d_host_set_subset_mask_search(flow2d_host_flow* h, int on)
{
    if (!h || (on != 0 && on != 1)) return 1;
    h->subset_mask_search = on == 1;
    return 0;
}

// Whether OpticalFlow2D::SubsetOptionsOk accepts the options with mask_search set: 1 only with a mask.  Needs no device.
HOST_API int flow2d_host_subset_mask_search_ok(const flow2d_host_subset_options* options)
{
    if (!options) return 0;
    auto subset = subset_options(*options);
    subset.mask_search = true;
    return OpticalFlow2D::SubsetOptionsOk(subset) ? 1 : 0;
}

// OpticalFlow2D::SubsetMinPixels: the default min_pixels of a radius.
HOST_API int flow2d_host_subset_min_pixels(int radius)
{
    OpticalFlow2D::SubsetOptions o;
    o.radius = radius;
    return OpticalFlow2D::SubsetMinPixels(o);
}

// OpticalFlow2D::RefineNodesDevice: device planes of the container's size; dev_out: the fourteen slots, each optional.  With a
// record (host) the call synchronises.  0 on success, 1 for a null or refused argument, 2 when the run failed.
HOST_API int flow2d_host_refine_nodes_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, void* dev_node_u0,
                                             void* dev_node_v0, int grid_radius, int spacing, const flow2d_host_subset_options* options,
                                             void* const* dev_out, flow2d_subset_record* record)
{
    if (!h || !dev_frame_0 || !dev_frame_1 || !dev_node_u0 || !dev_node_v0 || !options) return 1;
    const auto subset = subset_options(*options, h);
    if (!subset_accepted(subset, dev_out)) return 1;
    h->flow.timing_mode = 0;
    return h->flow.RefineNodesDevice(dp(dev_frame_0), dp(dev_frame_1), dp(dev_node_u0), dp(dev_node_v0), grid_radius, spacing, subset,
                                     subset_planes(dev_out), record)
               ? 0
               : 2;
}

// OpticalFlow2D::CorrelateSubsetDevice: the passes as for flow2d_host_correlate_multipass_device, then the refinement; dev_out as
// above, reports (optional) one per pass, record (optional).  Synchronises.  0, 1 or 2 as above.
HOST_API int flow2d_host_correlate_subset_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, float lo, float scale,
                                                 const int* passes, int count, float min_score, float threshold, float epsilon,
                                                 int min_neighbours, const flow2d_host_subset_options* options, void* dev_predictor_u,
                                                 void* dev_predictor_v, void* const* dev_out, OpticalFlow2D::CorrelationPassReport* reports,
                                                 flow2d_subset_record* record, void* dev_flow_u, void* dev_flow_v)
{
    const auto list = correlation_passes(passes, count);
    const auto validation = validation_options(threshold, epsilon, min_neighbours, 1, 1);
    if (!h || !dev_frame_0 || !dev_frame_1 || !options || count < 0 || (dev_flow_u == nullptr) != (dev_flow_v == nullptr) ||
        (dev_predictor_u == nullptr) != (dev_predictor_v == nullptr))
        return 1;
    const auto subset = subset_options(*options, h);
    if (!OpticalFlow2D::CorrelationPassesOk(h->width, h->height, lo, scale, list.data(), list.size(), min_score, validation) ||
        !subset_accepted(subset, dev_out))
        return 1;
    h->flow.timing_mode = 0;
    return h->flow.CorrelateSubsetDevice(dp(dev_frame_0), dp(dev_frame_1), lo, scale, list.data(), list.size(), min_score, validation, subset,
                                         dp(dev_predictor_u), dp(dev_predictor_v), subset_planes(dev_out), reports, record, dp(dev_flow_u),
                                         dp(dev_flow_v))
               ? 0
               : 2;
}

// OpticalFlow2D::CorrelateSubset on tight host images: nodes -- the fourteen slots as arrays (u and v needed, the gradients all or
// none, at order 2 the curvatures all or none) -- get the last pass's nw * nh floats each; options->mask: an image, which the object
// uploads once; the rest as for flow2d_host_correlate_multipass.
HOST_API int flow2d_host_correlate_subset(flow2d_host_flow* h, const float* frame_0, const float* frame_1, const int* passes, int count,
                                          float min_score, float threshold, float epsilon, int min_neighbours,
                                          const flow2d_host_subset_options* options, const float* predictor_u, const float* predictor_v,
                                          float* const* nodes, OpticalFlow2D::CorrelationPassReport* reports, flow2d_subset_record* record,
                                          float* flow_u, float* flow_v, float* lo_scale)
{
    const auto list = correlation_passes(passes, count);
    const auto validation = validation_options(threshold, epsilon, min_neighbours, 1, 1);
    if (!h || !frame_0 || !frame_1 || !options || !nodes || !nodes[0] || !nodes[1] || count < 0 ||
        (flow_u == nullptr) != (flow_v == nullptr) || (predictor_u == nullptr) != (predictor_v == nullptr))
        return 1;
    const auto subset = subset_options(*options, h);
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1);
    Data2D *pu = predictor_u ? im.In(predictor_u) : nullptr, *pv = predictor_v ? im.In(predictor_v) : nullptr;
    Data2D *fu = im.Out(flow_u, im.AfterSuccess), *fv = im.Out(flow_v, im.AfterSuccess);
    Data2D* mask = options->mask ? im.In(static_cast<const float*>(options->mask)) : nullptr;
    float lo = 0.f, scale = 1.f;
    OpticalFlow2D::CorrelationRange(*f0, *f1, lo, scale);
    if (!OpticalFlow2D::CorrelationPassesOk(h->width, h->height, lo, scale, list.data(), list.size(), min_score, validation) ||
        !subset_accepted(subset, nodes))
        return 1;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(h->width, h->height, list.back().radius, list.back().spacing, &nw, &nh);
    const int node_count = node_images(subset);
    std::vector<Data2D> images;
    for (int k = 0; k < node_count; ++k) images.emplace_back(nw, nh);
    Data2D* wanted[kSubsetSlots] = {};
    for (int k = 0; k < node_count; ++k) wanted[k] = nodes[k] ? &images[k] : nullptr;
    h->flow.CorrelateSubset(*f0, *f1, list.data(), list.size(), min_score, validation, subset, wanted, reports, record, fu, fv, pu, pv, mask);
    const int rc = im.Finish(h->flow);
    if (rc) return rc;
    for (int k = 0; k < node_count; ++k)
        if (nodes[k]) std::memcpy(nodes[k], images[k].DataPtr(), nw * nh * sizeof(float));
    if (lo_scale) {
        lo_scale[0] = lo;
        lo_scale[1] = scale;
    }
    return 0;
}

// ---- subset refinement over a sequence ------------------------------------------------------------------------------------------
namespace {
// (SequenceOptions::reference_every travels beside the entries' arguments the way SubsetOptions::interpolation does: kept in the
// object by flow2d_host_set_reference_every, so that the sequence entries keep the arguments callers built against)
OpticalFlow2D::SequenceOptions sequence_options(int fill, int min_state, int min_neighbours, float max_shift,
                                                const flow2d_host_flow* h = nullptr)
{
    OpticalFlow2D::SequenceOptions o;
    o.fill = fill;
    o.min_state = min_state;
    o.min_neighbours = min_neighbours;
    o.max_shift = max_shift;
    if (h) o.reference_every = h->reference_every;
    return o;
}
}  // namespace

// SequenceOptions::reference_every of every later sequence call of this object: 0 never (what a new object has), N >= 1 a new
// reference frame every N steps.  0 on success, 1 for a null object or a negative value, which changes nothing.
HOST_API int flow2d_host_set_reference_every(flow2d_host_flow* h, int every)
{
    if (!h || every < 0) return 1;
    h->reference_every = every;
    return 0;
}

// The composition records of the object's last sequence call, one per step (zero for a step measured against frame 0): up to
// `count` of them are copied into `records`; returns how many steps that call had.
HOST_API int flow2d_host_compose_records(const flow2d_host_flow* h, flow2d_compose_record* records, int count)
{
    if (!h) return 0;
    for (int k = 0; records && k < count && k < static_cast<int>(h->compose_records.size()); ++k) records[k] = h->compose_records[k];
    return static_cast<int>(h->compose_records.size());
}

// OpticalFlow2D::ComposeNodesDevice: dev_base -- seven device planes u, v, ux, uy, vx, vy, state --, dev_increment and dev_out -- the
// first eight slots of OpticalFlow2D::SubsetPlanes (u, v, ux, uy, vx, vy, score, state; the increment's score and the output's
// score and state optional).  With a record (host) the call synchronises.  0 on success, 1 for a null or refused argument, 2 when
// the run failed.
HOST_API int flow2d_host_compose_nodes_device(flow2d_host_flow* h, void* const* dev_base, void* const* dev_increment, int grid_radius,
                                              int spacing, int min_state, void* const* dev_out, flow2d_compose_record* record)
{
    if (!h || !dev_base || !dev_increment || !dev_out || min_state < 0 || min_state > 1) return 1;
    for (int k = 0; k < 7; ++k)
        if (!dev_base[k] || (k != 6 && !dev_increment[k]) || (k < 6 && !dev_out[k])) return 1;
    if (!dev_increment[7] || (dev_out[6] && !dev_increment[6])) return 1;
    OpticalFlow2D::SubsetPlanes base, increment, out;
    base = {dp(dev_base[0]), dp(dev_base[1]), dp(dev_base[2]), dp(dev_base[3]), dp(dev_base[4]), dp(dev_base[5]), 0, dp(dev_base[6])};
    increment = {dp(dev_increment[0]), dp(dev_increment[1]), dp(dev_increment[2]), dp(dev_increment[3]),
                 dp(dev_increment[4]), dp(dev_increment[5]), dp(dev_increment[6]), dp(dev_increment[7])};
    out = {dp(dev_out[0]), dp(dev_out[1]), dp(dev_out[2]), dp(dev_out[3]), dp(dev_out[4]), dp(dev_out[5]), dp(dev_out[6]), dp(dev_out[7])};
    h->flow.timing_mode = 0;
    return h->flow.ComposeNodesDevice(base, increment, grid_radius, spacing, min_state, out, record) ? 0 : 2;
}

// OpticalFlow2D::ComposeNodes on tight host arrays of nw * nh floats (the grid of the object's frames): base -- seven --, increment
// and nodes -- eight each, as above.
HOST_API int flow2d_host_compose_nodes(flow2d_host_flow* h, const float* const* base, const float* const* increment, int grid_radius,
                                       int spacing, int min_state, float* const* nodes, flow2d_compose_record* record)
{
    if (!h || !base || !increment || !nodes || min_state < 0 || min_state > 1) return 1;
    for (int k = 0; k < 7; ++k)
        if (!base[k] || (k != 6 && !increment[k]) || (k < 6 && !nodes[k])) return 1;
    if (!increment[7] || (nodes[6] && !increment[6])) return 1;
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(h->width, h->height, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) return 1;
    std::vector<Data2D> images;
    images.reserve(23);
    for (int k = 0; k < 23; ++k) images.emplace_back(nw, nh);
    Data2D *a[7], *b[8], *o[8];
    for (int k = 0; k < 7; ++k) {
        std::memcpy(images[k].DataPtr(), base[k], nw * nh * sizeof(float));
        a[k] = &images[k];
    }
    for (int k = 0; k < 8; ++k) {
        if (increment[k]) std::memcpy(images[7 + k].DataPtr(), increment[k], nw * nh * sizeof(float));
        b[k] = increment[k] ? &images[7 + k] : nullptr;
        o[k] = nodes[k] ? &images[15 + k] : nullptr;
    }
    h->flow.ComposeNodes(a, b, grid_radius, spacing, min_state, o, record);
    if (!h->flow.LastRunSucceeded()) return 2;
    for (int k = 0; k < 8; ++k)
        if (nodes[k]) std::memcpy(nodes[k], images[15 + k].DataPtr(), nw * nh * sizeof(float));
    return 0;
}

// OpticalFlow2D::UncertaintyOptionsOk: 1 when NodeUncertainty* accept the options (order 1 among it).  Needs no device.
HOST_API int flow2d_host_uncertainty_options_ok(const flow2d_host_subset_options* options, int min_state)
{
    return options && OpticalFlow2D::UncertaintyOptionsOk(subset_options(*options), min_state) ? 1 : 0;
}

// OpticalFlow2D::NodeUncertaintyDevice: dev_nodes -- seven device planes u, v, ux, uy, vx, vy, state of a first-order refinement, all
// needed --, dev_out -- eight device planes sigma_u, sigma_v, rho, sigma_ux, sigma_uy, sigma_vx, sigma_vy, noise, of which sigma_u and
// sigma_v are needed and the four gradient sigmas go all or none.  Of the options the radius, the mask with min_pixels and (beside
// them, in the object) the interpolation are used; order 2 is refused.  With a record (host) the call synchronises.  0 on success, 1
// for a null or refused argument, 2 when the run failed.
HOST_API int flow2d_host_node_uncertainty_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, void* const* dev_nodes,
                                                 int grid_radius, int spacing, const flow2d_host_subset_options* options, int min_state,
                                                 void* const* dev_out, flow2d_uncertainty_record* record)
{
    if (!h || !dev_frame_0 || !dev_frame_1 || !dev_nodes || !options || !dev_out || min_state < 0 || min_state > 1) return 1;
    for (int k = 0; k < 7; ++k)
        if (!dev_nodes[k]) return 1;
    const int gradients = (dev_out[3] != nullptr) + (dev_out[4] != nullptr) + (dev_out[5] != nullptr) + (dev_out[6] != nullptr);
    if (!dev_out[0] || !dev_out[1] || (gradients != 0 && gradients != 4)) return 1;
    const auto subset = subset_options(*options, h);
    if (!OpticalFlow2D::UncertaintyOptionsOk(subset, min_state)) return 1;
    OpticalFlow2D::SubsetPlanes nodes;
    nodes = {dp(dev_nodes[0]), dp(dev_nodes[1]), dp(dev_nodes[2]), dp(dev_nodes[3]), dp(dev_nodes[4]), dp(dev_nodes[5]), 0, dp(dev_nodes[6])};
    const OpticalFlow2D::UncertaintyPlanes out = {dp(dev_out[0]), dp(dev_out[1]), dp(dev_out[2]), dp(dev_out[3]),
                                                  dp(dev_out[4]), dp(dev_out[5]), dp(dev_out[6]), dp(dev_out[7])};
    h->flow.timing_mode = 0;
    return h->flow.NodeUncertaintyDevice(dp(dev_frame_0), dp(dev_frame_1), nodes, grid_radius, spacing, subset, min_state, out, record) ? 0 : 2;
}

// OpticalFlow2D::NodeUncertainty on tight host arrays: the frames, nodes -- seven arrays of nw * nh floats as above -- and out --
// eight, as above; options->mask: an image of the frames' size, which the object uploads.
HOST_API int flow2d_host_node_uncertainty(flow2d_host_flow* h, const float* frame_0, const float* frame_1, const float* const* nodes,
                                          int grid_radius, int spacing, const flow2d_host_subset_options* options, int min_state,
                                          float* const* out, flow2d_uncertainty_record* record)
{
    if (!h || !frame_0 || !frame_1 || !nodes || !options || !out || min_state < 0 || min_state > 1) return 1;
    for (int k = 0; k < 7; ++k)
        if (!nodes[k]) return 1;
    const int gradients = (out[3] != nullptr) + (out[4] != nullptr) + (out[5] != nullptr) + (out[6] != nullptr);
    if (!out[0] || !out[1] || (gradients != 0 && gradients != 4)) return 1;
    const auto subset = subset_options(*options, h);
    if (!OpticalFlow2D::UncertaintyOptionsOk(subset, min_state)) return 1;
    size_t nw = 0, nh = 0;
    if (flow2d_correlation_grid(h->width, h->height, grid_radius, spacing, &nw, &nh) != FLOW2D_OK) return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1);
    Data2D* mask = options->mask ? im.In(static_cast<const float*>(options->mask)) : nullptr;
    std::vector<Data2D> images;
    images.reserve(15);
    for (int k = 0; k < 15; ++k) images.emplace_back(nw, nh);
    Data2D *field[8], *wanted[8];
    for (int k = 0; k < 7; ++k) {
        std::memcpy(images[k].DataPtr(), nodes[k], nw * nh * sizeof(float));
        field[k < 6 ? k : 7] = &images[k];
    }
    field[6] = nullptr;  // (the score is not looked at)
    for (int k = 0; k < 8; ++k) wanted[k] = out[k] ? &images[7 + k] : nullptr;
    h->flow.NodeUncertainty(*f0, *f1, field, grid_radius, spacing, subset, min_state, wanted, record, mask);
    if (!h->flow.LastRunSucceeded()) return 2;
    for (int k = 0; k < 8; ++k)
        if (out[k]) std::memcpy(out[k], images[7 + k].DataPtr(), nw * nh * sizeof(float));
    return 0;
}

// OpticalFlow2D::SequenceOptionsOk.  Needs no device.
HOST_API int flow2d_host_sequence_options_ok(int fill, int min_state, int min_neighbours, float max_shift)
{
    return OpticalFlow2D::SequenceOptionsOk(sequence_options(fill, min_state, min_neighbours, max_shift)) ? 1 : 0;
}

// OpticalFlow2D::RefineNodesFromDevice: dev_start -- six device planes u, v, ux, uy, vx, vy, all needed (at order 2 the start's
// curvatures are 0); the rest as for flow2d_host_refine_nodes_device.
HOST_API int flow2d_host_refine_nodes_from_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, void* const* dev_start,
                                                  int grid_radius, int spacing, const flow2d_host_subset_options* options,
                                                  void* const* dev_out, flow2d_subset_record* record)
{
    if (!h || !dev_frame_0 || !dev_frame_1 || !dev_start || !options) return 1;
    const auto subset = subset_options(*options, h);
    if (!subset_accepted(subset, dev_out)) return 1;
    for (int k = 0; k < 6; ++k)
        if (!dev_start[k]) return 1;
    OpticalFlow2D::SubsetPlanes start;
    start = {dp(dev_start[0]), dp(dev_start[1]), dp(dev_start[2]), dp(dev_start[3]), dp(dev_start[4]), dp(dev_start[5]), 0, 0};
    h->flow.timing_mode = 0;
    return h->flow.RefineNodesFromDevice(dp(dev_frame_0), dp(dev_frame_1), start, grid_radius, spacing, subset, subset_planes(dev_out), record)
               ? 0
               : 2;
}

// the records as the facade takes them and hands them out
static_assert(sizeof(flow2d_host_subset_options) == 40, "flow2d_host_subset_options layout");
static_assert(sizeof(OpticalFlow2D::SequenceStepReport) == 64 + 64 * OpticalFlow2D::kSequenceMaxFill, "SequenceStepReport layout");

// OpticalFlow2D::CorrelateSubsetSequenceDevice: dev_frames -- `frames` device planes, the first the reference; dev_out -- the
// fourteen slots per step (of the first eight only the score may be null; at order 2 the curvatures all or none); dev_flows
// (optional) -- two per step, each pair optional; options->mask: every step uses it; reports (optional) one per pass of step 1,
// steps (optional) one per step.  Synchronises.  0, 1 or 2 as above.
HOST_API int flow2d_host_correlate_subset_sequence_device(flow2d_host_flow* h, void* const* dev_frames, int frames, float lo, float scale,
                                                          const int* passes, int count, float min_score, float threshold, float epsilon,
                                                          int min_neighbours, const flow2d_host_subset_options* options, int fill,
                                                          int min_state, int predict_neighbours, float sequence_max_shift,
                                                          void* const* dev_out, OpticalFlow2D::CorrelationPassReport* reports,
                                                          OpticalFlow2D::SequenceStepReport* steps, void* const* dev_flows)
{
    const auto list = correlation_passes(passes, count);
    const auto validation = validation_options(threshold, epsilon, min_neighbours, 1, 1);
    const auto sequence = sequence_options(fill, min_state, predict_neighbours, sequence_max_shift, h);
    if (!h || !dev_frames || frames < 2 || count < 0 || !dev_out || !options) return 1;
    const auto subset = subset_options(*options, h);
    const size_t n = static_cast<size_t>(frames), step_count = n - 1;
    if (!OpticalFlow2D::CorrelationPassesOk(h->width, h->height, lo, scale, list.data(), list.size(), min_score, validation) ||
        !subset_accepted(subset, dev_out, step_count) || !OpticalFlow2D::SequenceOptionsOk(sequence))
        return 1;
    std::vector<DevicePtr> frame_list(n), flow_list(2 * step_count, 0);
    for (size_t k = 0; k < n; ++k) {
        if (!dev_frames[k]) return 1;
        frame_list[k] = dp(dev_frames[k]);
    }
    std::vector<OpticalFlow2D::SubsetPlanes> out(step_count);
    for (size_t k = 0; k < step_count; ++k) {
        void* const* step = dev_out + kSubsetSlots * k;
        out[k] = subset_planes(step);
        for (int c = 0; c < 8; ++c)
            if (c != 6 && !step[c]) return 1;
        for (int c = 0; dev_flows && c < 2; ++c) flow_list[2 * k + c] = dp(dev_flows[2 * k + c]);
        if ((flow_list[2 * k] == 0) != (flow_list[2 * k + 1] == 0)) return 1;
    }
    h->flow.timing_mode = 0;
    h->compose_records.assign(step_count, flow2d_compose_record{});
    return h->flow.CorrelateSubsetSequenceDevice(frame_list.data(), n, lo, scale, list.data(), list.size(), min_score, validation, subset,
                                                 sequence, out.data(), reports, steps, dev_flows ? flow_list.data() : nullptr,
                                                 h->compose_records.data())
               ? 0
               : 2;
}

// OpticalFlow2D::CorrelateSubsetSequence on tight host images: frames -- `count_frames` images; nodes -- the fourteen slots per step
// as arrays, which get the last pass's nw * nh floats each (of the first eight only a score may be null); flows (optional) -- two
// images per step, each pair optional; options->mask: an image, uploaded once for all steps.
HOST_API int flow2d_host_correlate_subset_sequence(flow2d_host_flow* h, const float* const* frames, int count_frames, const int* passes,
                                                   int count, float min_score, float threshold, float epsilon, int min_neighbours,
                                                   const flow2d_host_subset_options* options, int fill, int min_state,
                                                   int predict_neighbours, float sequence_max_shift, float* const* nodes,
                                                   OpticalFlow2D::CorrelationPassReport* reports, OpticalFlow2D::SequenceStepReport* steps,
                                                   float* const* flows, float* lo_scale)
{
    const auto list = correlation_passes(passes, count);
    const auto validation = validation_options(threshold, epsilon, min_neighbours, 1, 1);
    const auto sequence = sequence_options(fill, min_state, predict_neighbours, sequence_max_shift, h);
    if (!h || !frames || count_frames < 2 || !nodes || count < 0 || !options) return 1;
    const auto subset = subset_options(*options, h);
    const size_t n = static_cast<size_t>(count_frames), step_count = n - 1;
    for (size_t k = 0; k < n; ++k)
        if (!frames[k]) return 1;
    for (size_t k = 0; k < step_count; ++k) {
        for (int c = 0; c < 8; ++c)
            if (c != 6 && !nodes[kSubsetSlots * k + c]) return 1;
        if (flows && (flows[2 * k] == nullptr) != (flows[2 * k + 1] == nullptr)) return 1;
    }
    HostImages im(h);
    std::vector<Data2D*> in(n), flow_images(2 * step_count, nullptr);
    for (size_t k = 0; k < n; ++k) in[k] = im.In(frames[k]);
    for (size_t k = 0; flows && k < 2 * step_count; ++k) flow_images[k] = im.Out(flows[k], im.AfterSuccess);
    Data2D* mask = options->mask ? im.In(static_cast<const float*>(options->mask)) : nullptr;
    float lo = 0.f, scale = 1.f;
    OpticalFlow2D::CorrelationRange(*in[0], *in[1], lo, scale);
    if (!OpticalFlow2D::CorrelationPassesOk(h->width, h->height, lo, scale, list.data(), list.size(), min_score, validation) ||
        !subset_accepted(subset, nodes, step_count) || !OpticalFlow2D::SequenceOptionsOk(sequence))
        return 1;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(h->width, h->height, list.back().radius, list.back().spacing, &nw, &nh);
    // image per_step * k + c is slot c of step k: OpticalFlow2D::CorrelateSubsetSequence takes the steps' images side by side
    const size_t per_step = static_cast<size_t>(node_images(subset));
    auto slot = [&](size_t image) { return nodes[kSubsetSlots * (image / per_step) + image % per_step]; };
    std::vector<Data2D> images;
    images.reserve(per_step * step_count);
    for (size_t k = 0; k < per_step * step_count; ++k) images.emplace_back(nw, nh);
    std::vector<Data2D*> wanted(per_step * step_count);
    for (size_t k = 0; k < per_step * step_count; ++k) wanted[k] = slot(k) ? &images[k] : nullptr;
    h->compose_records.assign(step_count, flow2d_compose_record{});
    h->flow.CorrelateSubsetSequence(in.data(), n, list.data(), list.size(), min_score, validation, subset, sequence, wanted.data(), reports,
                                    steps, flows ? flow_images.data() : nullptr, mask, h->compose_records.data());
    const int rc = im.Finish(h->flow);
    if (rc) return rc;
    for (size_t k = 0; k < per_step * step_count; ++k)
        if (slot(k)) std::memcpy(slot(k), images[k].DataPtr(), nw * nh * sizeof(float));
    if (lo_scale) {
        lo_scale[0] = lo;
        lo_scale[1] = scale;
    }
    return 0;
}

// ---- strain on the node grid ---------------------------------------------------------------------------------------------------
namespace {
// The entries below were there before the robust fit, and their argument lists stay: its scale and passes travel beside them, kept
// in the object by flow2d_host_set_strain_robust, and the diagnostic planes of the next call by flow2d_host_set_strain_diagnostics.
OpticalFlow2D::StrainOptions strain_options(int window, int order, int min_nodes, int min_state, int measure,
                                            const flow2d_host_flow* h = nullptr)
{
    OpticalFlow2D::StrainOptions o;
    o.window = window;
    o.order = order;
    o.min_nodes = min_nodes;
    o.min_state = min_state;
    o.measure = measure;
    if (h) {
        o.robust_sigma = h->strain_sigma;
        o.robust_iterations = h->strain_iterations;
        if (h->strain_weighted) {
            o.weighted = true;
            o.sigma_floor = h->strain_floor;
            o.weight_threshold = h->strain_threshold;
            o.robust_iterations = h->strain_weight_iterations;
        }
    }
    return o;
}

// The diagnostic planes handed in for this call (three per step, or none), taken out of the object.
std::vector<void*> take_diagnostics(flow2d_host_flow* h, size_t step_count, bool& ok)
{
    std::vector<void*> given;
    given.swap(h->strain_diagnostics);
    ok = given.empty() || given.size() == 3 * step_count;
    return given;
}
}  // namespace

// OpticalFlow2D::StrainOptionsOk with the robust fields.  Needs no device.
HOST_API int flow2d_host_strain_robust_options_ok(int window, int order, int min_nodes, int min_state, int measure, float sigma,
                                                  int iterations)
{
    auto o = strain_options(window, order, min_nodes, min_state, measure);
    o.robust_sigma = sigma;
    o.robust_iterations = iterations;
    return OpticalFlow2D::StrainOptionsOk(o) ? 1 : 0;
}

// StrainOptions::robust_sigma and robust_iterations of the node-strain calls that follow; sigma 0 = the plain fit (the default).
// 1 for a scale that is negative or not finite, or iterations outside 0 .. FLOW2D_NODE_STRAIN_MAX_ITERATIONS.
HOST_API int flow2d_host_set_strain_robust(flow2d_host_flow* h, float sigma, int iterations)
{
    if (!h || !(std::isfinite(sigma) && sigma >= 0.f) || iterations < 0 || iterations > FLOW2D_NODE_STRAIN_MAX_ITERATIONS) return 1;
    h->strain_sigma = sigma;
    h->strain_iterations = iterations;
    return 0;
}

// OpticalFlow2D::StrainOptionsOk with the weighted fields (and a robust scale, which they exclude).  Needs no device.
HOST_API int flow2d_host_strain_weighted_options_ok(int window, int order, int min_nodes, int min_state, int measure, float robust_sigma,
                                                    float sigma_floor, float threshold, int iterations)
{
    auto o = strain_options(window, order, min_nodes, min_state, measure);
    o.robust_sigma = robust_sigma;
    o.weighted = true;
    o.sigma_floor = sigma_floor;
    o.weight_threshold = threshold;
    o.robust_iterations = iterations;
    return OpticalFlow2D::StrainOptionsOk(o) ? 1 : 0;
}

// StrainOptions::weighted, sigma_floor, weight_threshold and the passes of the weighted node-strain calls that follow
// (flow2d_host_node_strain_weighted*); weighted 0 = off (the default).  1 for a floor or threshold that is negative or not finite,
// or iterations outside 0 .. FLOW2D_NODE_STRAIN_MAX_ITERATIONS.  A robust scale set beside it makes those calls fail: the two
// exclude each other.
HOST_API int flow2d_host_set_strain_weighting(flow2d_host_flow* h, int weighted, float sigma_floor, float threshold, int iterations)
{
    if (!h || !(std::isfinite(sigma_floor) && sigma_floor >= 0.f) || !(std::isfinite(threshold) && threshold >= 0.f) || iterations < 0 ||
        iterations > FLOW2D_NODE_STRAIN_MAX_ITERATIONS)
        return 1;
    h->strain_weighted = weighted != 0;
    h->strain_floor = sigma_floor;
    h->strain_threshold = threshold;
    h->strain_weight_iterations = iterations;
    return 0;
}

// The diagnostic planes of the NEXT flow2d_host_node_strain (tight host arrays of nw * nh floats) or
// flow2d_host_node_strain_device (device planes) call: three per step -- residual, rejected, centre --, each optional; that call
// must have `steps` steps and a robust scale, and forgets them.  planes == NULL or steps == 0 withdraws them.
HOST_API int flow2d_host_set_strain_diagnostics(flow2d_host_flow* h, void* const* planes, int steps)
{
    if (!h || steps < 0) return 1;
    h->strain_diagnostics.clear();
    if (planes && steps > 0) h->strain_diagnostics.assign(planes, planes + 3 * static_cast<size_t>(steps));
    return 0;
}

// OpticalFlow2D::StrainOptionsOk.  Needs no device.
HOST_API int flow2d_host_strain_options_ok(int window, int order, int min_nodes, int min_state, int measure)
{
    return OpticalFlow2D::StrainOptionsOk(strain_options(window, order, min_nodes, min_state, measure)) ? 1 : 0;
}

// OpticalFlow2D::NodeStrainDevice: dev_nodes -- seven device planes per step (u, v, ux, uy, vx, vy, state; u and v needed, the
// gradients all or none, the state optional), dev_planes -- nine per step in the order of flow2d_deformation_planes, each optional
// (the array may be null with stats); stats (host, optional) -- one record per step: with it the call synchronises.  0, 1 or 2.
HOST_API int flow2d_host_node_strain_device(flow2d_host_flow* h, void* const* dev_nodes, int steps, size_t nw, size_t nh, int spacing,
                                            int window, int order, int min_nodes, int min_state, int measure, void* const* dev_planes,
                                            flow2d_deformation_stats* stats)
{
    const auto strain = strain_options(window, order, min_nodes, min_state, measure, h);
    if (!h) return 1;
    bool diagnostics_ok = false;
    const std::vector<void*> given_diagnostics = take_diagnostics(h, steps < 1 ? 0 : static_cast<size_t>(steps), diagnostics_ok);
    if (!diagnostics_ok || (!given_diagnostics.empty() && strain.robust_sigma == 0.f)) return 1;
    if (!dev_nodes || steps < 1 || (!dev_planes && !stats && given_diagnostics.empty()) || !OpticalFlow2D::StrainOptionsOk(strain)) return 1;
    const size_t step_count = static_cast<size_t>(steps);
    std::vector<DevicePtr> diagnostics;
    for (void* q : given_diagnostics) diagnostics.push_back(dp(q));
    std::vector<OpticalFlow2D::SubsetPlanes> fields(step_count);
    std::vector<DevicePtr> planes(9 * step_count, 0);
    for (size_t k = 0; k < step_count; ++k) {
        void* const* q = dev_nodes + 7 * k;
        if (!q[0] || !q[1]) return 1;
        fields[k] = {dp(q[0]), dp(q[1]), dp(q[2]), dp(q[3]), dp(q[4]), dp(q[5]), 0, dp(q[6])};
        for (int c = 0; dev_planes && c < 9; ++c) planes[9 * k + c] = dp(dev_planes[9 * k + c]);
    }
    h->flow.timing_mode = 0;
    return h->flow.NodeStrainDevice(fields.data(), step_count, nw, nh, spacing, strain, dev_planes ? planes.data() : nullptr, stats,
                                    diagnostics.empty() ? nullptr : diagnostics.data())
               ? 0
               : 2;
}

// OpticalFlow2D::NodeStrain on tight host arrays of nw * nh floats: nodes -- seven per step, planes -- nine per step, as above.
HOST_API int flow2d_host_node_strain(flow2d_host_flow* h, const float* const* nodes, int steps, size_t nw, size_t nh, int spacing, int window,
                                     int order, int min_nodes, int min_state, int measure, float* const* planes,
                                     flow2d_deformation_stats* stats)
{
    const auto strain = strain_options(window, order, min_nodes, min_state, measure, h);
    if (!h) return 1;
    bool diagnostics_ok = false;
    const std::vector<void*> diagnostics = take_diagnostics(h, steps < 1 ? 0 : static_cast<size_t>(steps), diagnostics_ok);
    if (!diagnostics_ok || (!diagnostics.empty() && strain.robust_sigma == 0.f)) return 1;
    if (!nodes || steps < 1 || nw == 0 || nh == 0 || (!planes && !stats && diagnostics.empty()) || !OpticalFlow2D::StrainOptionsOk(strain))
        return 1;
    const size_t step_count = static_cast<size_t>(steps);
    std::vector<Data2D> in, out, diag;
    in.reserve(7 * step_count);
    out.reserve(9 * step_count);
    diag.reserve(3 * step_count);
    std::vector<Data2D*> wanted_diagnostics(diagnostics.size(), nullptr);
    for (size_t k = 0; k < diagnostics.size(); ++k) {
        diag.emplace_back(nw, nh);
        if (diagnostics[k]) wanted_diagnostics[k] = &diag[k];
    }
    std::vector<Data2D*> given(7 * step_count, nullptr), wanted(9 * step_count, nullptr);
    for (size_t k = 0; k < 7 * step_count; ++k) {
        in.emplace_back(nw, nh);
        if (!nodes[k]) continue;
        std::memcpy(in[k].DataPtr(), nodes[k], nw * nh * sizeof(float));
        given[k] = &in[k];
    }
    for (size_t k = 0; k < 9 * step_count; ++k) {
        out.emplace_back(nw, nh);
        if (planes && planes[k]) wanted[k] = &out[k];
    }
    for (size_t k = 0; k < step_count; ++k)
        if (!given[7 * k] || !given[7 * k + 1]) return 1;
    h->flow.NodeStrain(given.data(), step_count, spacing, strain, planes ? wanted.data() : nullptr, stats,
                       diagnostics.empty() ? nullptr : wanted_diagnostics.data());
    if (!h->flow.LastRunSucceeded()) return 2;
    for (size_t k = 0; k < diagnostics.size(); ++k)
        if (diagnostics[k]) std::memcpy(diagnostics[k], diag[k].DataPtr(), nw * nh * sizeof(float));
    for (size_t k = 0; planes && k < 9 * step_count; ++k)
        if (planes[k]) std::memcpy(planes[k], out[k].DataPtr(), nw * nh * sizeof(float));
    return 0;
}

// OpticalFlow2D::NodeStrainDevice, the weighted form (after flow2d_host_set_strain_weighting): dev_nodes and dev_planes as for
// flow2d_host_node_strain_device, dev_uncertainty -- two device planes per step, sigma_u and sigma_v, both needed --, dev_sigmas --
// nine per step in the order of flow2d_strain_sigma_planes, each optional, the array may be null.  The diagnostic planes of
// flow2d_host_set_strain_diagnostics go with it.  0, 1 or 2.
HOST_API int flow2d_host_node_strain_weighted_device(flow2d_host_flow* h, void* const* dev_nodes, void* const* dev_uncertainty, int steps,
                                                     size_t nw, size_t nh, int spacing, int window, int order, int min_nodes, int min_state,
                                                     int measure, void* const* dev_planes, void* const* dev_sigmas,
                                                     flow2d_deformation_stats* stats)
{
    const auto strain = strain_options(window, order, min_nodes, min_state, measure, h);
    if (!h) return 1;
    bool diagnostics_ok = false;
    const std::vector<void*> given_diagnostics = take_diagnostics(h, steps < 1 ? 0 : static_cast<size_t>(steps), diagnostics_ok);
    if (!diagnostics_ok || !strain.weighted) return 1;
    if (!dev_nodes || !dev_uncertainty || steps < 1 || (!dev_planes && !dev_sigmas && !stats && given_diagnostics.empty()) ||
        !OpticalFlow2D::StrainOptionsOk(strain))
        return 1;
    const size_t step_count = static_cast<size_t>(steps);
    std::vector<DevicePtr> diagnostics, uncertainty(2 * step_count, 0), planes(9 * step_count, 0);
    for (void* q : given_diagnostics) diagnostics.push_back(dp(q));
    std::vector<OpticalFlow2D::SubsetPlanes> fields(step_count);
    std::vector<OpticalFlow2D::StrainSigmaPlanes> sigmas(step_count);
    for (size_t k = 0; k < step_count; ++k) {
        void* const* q = dev_nodes + 7 * k;
        if (!q[0] || !q[1] || !dev_uncertainty[2 * k] || !dev_uncertainty[2 * k + 1]) return 1;
        fields[k] = {dp(q[0]), dp(q[1]), dp(q[2]), dp(q[3]), dp(q[4]), dp(q[5]), 0, dp(q[6])};
        uncertainty[2 * k] = dp(dev_uncertainty[2 * k]);
        uncertainty[2 * k + 1] = dp(dev_uncertainty[2 * k + 1]);
        for (int c = 0; dev_planes && c < 9; ++c) planes[9 * k + c] = dp(dev_planes[9 * k + c]);
        if (dev_sigmas) {
            void* const* e = dev_sigmas + 9 * k;
            sigmas[k] = {dp(e[0]), dp(e[1]), dp(e[2]), dp(e[3]), dp(e[4]), dp(e[5]), dp(e[6]), dp(e[7]), dp(e[8])};
        }
    }
    h->flow.timing_mode = 0;
    return h->flow.NodeStrainDevice(fields.data(), step_count, nw, nh, spacing, strain, uncertainty.data(),
                                    dev_planes ? planes.data() : nullptr, stats, diagnostics.empty() ? nullptr : diagnostics.data(),
                                    dev_sigmas ? sigmas.data() : nullptr)
               ? 0
               : 2;
}

// OpticalFlow2D::NodeStrain, the weighted form, on tight host arrays of nw * nh floats: nodes -- seven per step, uncertainty -- two per
// step, planes -- nine per step, sigmas -- nine per step, as above.
HOST_API int flow2d_host_node_strain_weighted(flow2d_host_flow* h, const float* const* nodes, const float* const* uncertainty, int steps,
                                              size_t nw, size_t nh, int spacing, int window, int order, int min_nodes, int min_state,
                                              int measure, float* const* planes, float* const* sigmas, flow2d_deformation_stats* stats)
{
    const auto strain = strain_options(window, order, min_nodes, min_state, measure, h);
    if (!h) return 1;
    bool diagnostics_ok = false;
    const std::vector<void*> diagnostics = take_diagnostics(h, steps < 1 ? 0 : static_cast<size_t>(steps), diagnostics_ok);
    if (!diagnostics_ok || !strain.weighted) return 1;
    if (!nodes || !uncertainty || steps < 1 || nw == 0 || nh == 0 || (!planes && !sigmas && !stats && diagnostics.empty()) ||
        !OpticalFlow2D::StrainOptionsOk(strain))
        return 1;
    const size_t step_count = static_cast<size_t>(steps);
    // the images of one kind: `per` per step, copied from `from` (read) or handed back into `to` (written), null = absent
    struct Kind {
        size_t per;
        const float* const* from;
        void* const* to;
        std::vector<Data2D> images;
        std::vector<Data2D*> given;
    };
    Kind kinds[5] = {{7, nodes, nullptr, {}, {}},
                     {2, uncertainty, nullptr, {}, {}},
                     {9, nullptr, reinterpret_cast<void* const*>(planes), {}, {}},
                     {3, nullptr, diagnostics.empty() ? nullptr : diagnostics.data(), {}, {}},
                     {9, nullptr, reinterpret_cast<void* const*>(sigmas), {}, {}}};
    for (Kind& kind : kinds) {
        const size_t count = kind.per * step_count;
        kind.images.reserve(count);
        kind.given.assign(count, nullptr);
        for (size_t k = 0; k < count; ++k) {
            kind.images.emplace_back(nw, nh);
            if (kind.from && kind.from[k]) {
                std::memcpy(kind.images[k].DataPtr(), kind.from[k], nw * nh * sizeof(float));
                kind.given[k] = &kind.images[k];
            }
            if (kind.to && kind.to[k]) kind.given[k] = &kind.images[k];
        }
    }
    for (size_t k = 0; k < step_count; ++k)
        if (!kinds[0].given[7 * k] || !kinds[0].given[7 * k + 1] || !kinds[1].given[2 * k] || !kinds[1].given[2 * k + 1]) return 1;
    h->flow.NodeStrain(kinds[0].given.data(), step_count, spacing, strain, kinds[1].given.data(), planes ? kinds[2].given.data() : nullptr,
                       stats, diagnostics.empty() ? nullptr : kinds[3].given.data(), sigmas ? kinds[4].given.data() : nullptr);
    if (!h->flow.LastRunSucceeded()) return 2;
    for (Kind& kind : kinds)
        for (size_t k = 0; kind.to && k < kind.per * step_count; ++k)
            if (kind.to[k]) std::memcpy(kind.to[k], kind.images[k].DataPtr(), nw * nh * sizeof(float));
    return 0;
}

// ---- the pyramid started from a prior flow ------------------------------------------------------------------------------------
// OpticalFlow2D::PriorReport as the facade hands it out
struct flow2d_host_prior_report {
    size_t start_level, levels_run;
    unsigned long long not_finite;
};

namespace {
void Report(flow2d_host_prior_report* out, const OpticalFlow2D::PriorReport& r)
{
    if (out) *out = {r.start_level, r.levels_run, r.not_finite};
}
}  // namespace

// OpticalFlow2D::PriorStartLevel: the level a pyramid from a prior starts at (prior_level -1: the rule from `reach`).  0 and *start
// written, or 1 when the arguments are refused.  Needs no device.
HOST_API int flow2d_host_prior_start_level(size_t width, size_t height, size_t warp_levels_count, float warp_scale_factor, float reach,
                                           int prior_level, size_t* start)
{
    return OpticalFlow2D::PriorStartLevel(width, height, warp_levels_count, warp_scale_factor, reach, prior_level, start) ? 0 : 1;
}

// OpticalFlow2D::ComputeFlowFromPriorDevice: frames, prior and flow in pitched device containers.  reach / prior_level: the bag keys
// prior_reach / prior_level (-1: not given).  With `report` the call synchronises, otherwise it only queues.  0 on success.
HOST_API int flow2d_host_compute_flow_from_prior_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, void* dev_prior_u,
                                                        void* dev_prior_v, void* dev_flow_u, void* dev_flow_v,
                                                        const flow2d_host_params* params, float reach, int prior_level,
                                                        flow2d_host_prior_report* report)
{
    if (!h || !params) return 1;
    PriorBag bag(*params, reach, prior_level);
    h->flow.timing_mode = 0;
    OpticalFlow2D::PriorReport r;
    if (!h->flow.ComputeFlowFromPriorDevice(dp(dev_frame_0), dp(dev_frame_1), dp(dev_prior_u), dp(dev_prior_v), dp(dev_flow_u),
                                            dp(dev_flow_v), bag, report ? &r : nullptr))
        return 2;
    Report(report, r);
    return 0;
}

// OpticalFlow2D::ComputeFlowFromPrior on tight host images.  0 on success, 2 when the run delivered no flow.
HOST_API int flow2d_host_compute_flow_from_prior(flow2d_host_flow* h, const float* frame_0, const float* frame_1, const float* prior_u,
                                                 const float* prior_v, float* flow_u, float* flow_v, const flow2d_host_params* params,
                                                 float reach, int prior_level, flow2d_host_prior_report* report, float* total_ms)
{
    if (!h || !frame_0 || !frame_1 || !prior_u || !prior_v || !flow_u || !flow_v || !params) return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *pu = im.In(prior_u), *pv = im.In(prior_v);
    Data2D *u = im.Out(flow_u, im.Always), *v = im.Out(flow_v, im.Always);
    PriorBag bag(*params, reach, prior_level);
    OpticalFlow2D::PriorReport r;
    h->flow.ComputeFlowFromPrior(*f0, *f1, *pu, *pv, *u, *v, bag, &r);
    Report(report, r);
    return im.Finish(h->flow, total_ms);
}

// OpticalFlow2D::ComputeFlowCorrelationSeededDevice: the correlation's arguments as for flow2d_host_correlate_device; node planes,
// records and the copy of the expanded field (dev_prior_u / dev_prior_v) optional.  Synchronises.  0 on success, 1 for a null or
// refused argument, 2 when the run failed.
HOST_API int flow2d_host_compute_flow_correlation_seeded_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, float lo,
                                                                float scale, int radius, int range, int spacing, float min_score,
                                                                void* dev_flow_u, void* dev_flow_v, const flow2d_host_params* params,
                                                                float reach, int prior_level, void* dev_node_u, void* dev_node_v,
                                                                void* dev_node_score, flow2d_correlation_record* record,
                                                                flow2d_host_prior_report* report, void* dev_prior_u, void* dev_prior_v)
{
    if (!h || !params || !dev_frame_0 || !dev_frame_1 || !dev_flow_u || !dev_flow_v || (dev_prior_u == nullptr) != (dev_prior_v == nullptr) ||
        !OpticalFlow2D::CorrelationArgsOk(h->width, h->height, lo, scale, radius, range, spacing, min_score))
        return 1;
    PriorBag bag(*params, reach, prior_level);
    h->flow.timing_mode = 0;
    OpticalFlow2D::PriorReport r;
    if (!h->flow.ComputeFlowCorrelationSeededDevice(dp(dev_frame_0), dp(dev_frame_1), lo, scale, radius, range, spacing, min_score,
                                                    dp(dev_flow_u), dp(dev_flow_v), bag, dp(dev_node_u), dp(dev_node_v), dp(dev_node_score),
                                                    record, &r, dp(dev_prior_u), dp(dev_prior_v)))
        return 2;
    Report(report, r);
    return 0;
}

// OpticalFlow2D::ComputeFlowCorrelationSeeded on tight host images: node_u / node_v / node_score (each optional) get nw * nh floats,
// prior_u / prior_v (optional, both or neither) the expanded field, lo_scale (optional) the two numbers of CorrelationRange.
HOST_API int flow2d_host_compute_flow_correlation_seeded(flow2d_host_flow* h, const float* frame_0, const float* frame_1, int radius,
                                                         int range, int spacing, float min_score, float* flow_u, float* flow_v,
                                                         const flow2d_host_params* params, float reach, int prior_level, float* node_u,
                                                         float* node_v, float* node_score, flow2d_correlation_record* record,
                                                         flow2d_host_prior_report* report, float* prior_u, float* prior_v,
                                                         float* lo_scale, float* total_ms)
{
    size_t nw = 0, nh = 0;
    if (!h || !params || !frame_0 || !frame_1 || !flow_u || !flow_v || (prior_u == nullptr) != (prior_v == nullptr) ||
        flow2d_correlation_grid(h->width, h->height, radius, spacing, &nw, &nh) != FLOW2D_OK)
        return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1);
    Data2D *u = im.Out(flow_u, im.Always), *v = im.Out(flow_v, im.Always);
    Data2D *pu = im.Out(prior_u, im.AfterSuccess), *pv = im.Out(prior_v, im.AfterSuccess);
    float lo = 0.f, scale = 1.f;
    OpticalFlow2D::CorrelationRange(*f0, *f1, lo, scale);
    if (!OpticalFlow2D::CorrelationArgsOk(h->width, h->height, lo, scale, radius, range, spacing, min_score)) return 1;
    Data2D nodes[3] = {Data2D(nw, nh), Data2D(nw, nh), Data2D(nw, nh)};
    PriorBag bag(*params, reach, prior_level);
    OpticalFlow2D::PriorReport r;
    h->flow.ComputeFlowCorrelationSeeded(*f0, *f1, radius, range, spacing, min_score, *u, *v, bag, node_u ? &nodes[0] : nullptr,
                                         node_v ? &nodes[1] : nullptr, node_score ? &nodes[2] : nullptr, record, &r, pu, pv);
    const int rc = im.Finish(h->flow, total_ms);
    if (rc) return rc;
    Report(report, r);
    float* dst[3] = {node_u, node_v, node_score};
    for (int k = 0; k < 3; ++k)
        if (dst[k]) std::memcpy(dst[k], nodes[k].DataPtr(), nw * nh * sizeof(float));
    if (lo_scale) {
        lo_scale[0] = lo;
        lo_scale[1] = scale;
    }
    return 0;
}

// ---- warm starts: the previous pair's flow as the prior ----------------------------------------------------------------------------
// OpticalFlow2D::WarmOptions / WarmReport as the facade takes and hands them out
struct flow2d_host_warm_options {
    int fill_passes;
    float photo_scale;
    float tail;  // < 0: no adaptation
};
struct flow2d_host_warm_report {
    int mode;   // 0 unseeded, 1 seeded, 2 redone
    int reach;  // adaptive mode: the reach the pair was seeded with, 0 unseeded
    size_t start_level, levels_run;
    unsigned long long not_finite;
    flow2d_propagate_record propagation;
    double share[3];
};

namespace {
OpticalFlow2D::WarmOptions Options(const flow2d_host_warm_options& o)
{
    OpticalFlow2D::WarmOptions out;
    out.fill_passes = o.fill_passes;
    out.photo_scale = o.photo_scale;
    out.tail = o.tail;
    return out;
}
void Report(flow2d_host_warm_report* out, const OpticalFlow2D::WarmReport* r, size_t count)
{
    for (size_t k = 0; out && k < count; ++k) {
        out[k] = {r[k].mode, r[k].reach, r[k].prior.start_level, r[k].prior.levels_run, r[k].prior.not_finite, r[k].propagation,
                  {r[k].share[0], r[k].share[1], r[k].share[2]}};
    }
}
}  // namespace

// OpticalFlow2D::WarmNextReach: the adaptive rule of a warm sequence over one record (above: the counts beyond 1, 2, 3 px).  0 and
// *redo / *next_reach written, or 1 when the arguments are refused.  Needs no device.
HOST_API int flow2d_host_warm_next_reach(unsigned long long count, const unsigned long long* above, float tail, int reach_used, int* redo,
                                         int* next_reach)
{
    bool again = false;
    int next = 0;
    if (!redo || !next_reach || !OpticalFlow2D::WarmNextReach(count, above, tail, reach_used, &again, &next)) return 1;
    *redo = again ? 1 : 0;
    *next_reach = next;
    return 0;
}

// OpticalFlow2D::WarmOptionsOk: 1 when the options are acceptable.  Needs no device.
HOST_API int flow2d_host_warm_options_ok(const flow2d_host_warm_options* options)
{
    return options && OpticalFlow2D::WarmOptionsOk(Options(*options)) ? 1 : 0;
}

// OpticalFlow2D::PropagateFlowDevice: planes in pitched device containers; mask and the two frames optional.  With `record` the call
// synchronises, otherwise it only queues.  0 on success.
HOST_API int flow2d_host_propagate_flow_device(flow2d_host_flow* h, void* dev_flow_u, void* dev_flow_v, void* dev_mask, void* dev_frame_from,
                                               void* dev_frame_to, float step, const flow2d_host_warm_options* options, void* dev_out_u,
                                               void* dev_out_v, flow2d_propagate_record* record)
{
    if (!h || !options) return 1;
    return h->flow.PropagateFlowDevice(dp(dev_flow_u), dp(dev_flow_v), dp(dev_mask), dp(dev_frame_from), dp(dev_frame_to), step,
                                       Options(*options), dp(dev_out_u), dp(dev_out_v), record)
               ? 0
               : 2;
}

// OpticalFlow2D::ComputeFlowFromPreviousDevice.  reach / prior_level as for flow2d_host_compute_flow_from_prior_device.  With `report`
// the call synchronises.  0 on success.
HOST_API int flow2d_host_compute_flow_from_previous_device(flow2d_host_flow* h, void* dev_frame_0, void* dev_frame_1, void* dev_prev_u,
                                                           void* dev_prev_v, void* dev_prev_mask, void* dev_prev_frame, void* dev_flow_u,
                                                           void* dev_flow_v, const flow2d_host_params* params, float reach, int prior_level,
                                                           const flow2d_host_warm_options* options, flow2d_host_warm_report* report)
{
    if (!h || !params || !options) return 1;
    PriorBag bag(*params, reach, prior_level);
    h->flow.timing_mode = 0;
    OpticalFlow2D::WarmReport r;
    if (!h->flow.ComputeFlowFromPreviousDevice(dp(dev_frame_0), dp(dev_frame_1), dp(dev_prev_u), dp(dev_prev_v), dp(dev_prev_mask),
                                               dp(dev_prev_frame), dp(dev_flow_u), dp(dev_flow_v), bag, Options(*options),
                                               report ? &r : nullptr))
        return 2;
    Report(report, &r, 1);
    return 0;
}

// OpticalFlow2D::ComputeFlowFromPrevious on tight host images; prev_mask and prev_frame optional.
HOST_API int flow2d_host_compute_flow_from_previous(flow2d_host_flow* h, const float* frame_0, const float* frame_1, const float* prev_u,
                                                    const float* prev_v, const float* prev_mask, const float* prev_frame, float* flow_u,
                                                    float* flow_v, const flow2d_host_params* params, float reach, int prior_level,
                                                    const flow2d_host_warm_options* options, flow2d_host_warm_report* report,
                                                    float* total_ms)
{
    if (!h || !frame_0 || !frame_1 || !prev_u || !prev_v || !flow_u || !flow_v || !params || !options) return 1;
    HostImages im(h);
    Data2D *f0 = im.In(frame_0), *f1 = im.In(frame_1), *pu = im.In(prev_u), *pv = im.In(prev_v);
    Data2D *mask = prev_mask ? im.In(prev_mask) : nullptr, *frame = prev_frame ? im.In(prev_frame) : nullptr;
    Data2D *u = im.Out(flow_u, im.Always), *v = im.Out(flow_v, im.Always);
    PriorBag bag(*params, reach, prior_level);
    OpticalFlow2D::WarmReport r;
    h->flow.ComputeFlowFromPrevious(*f0, *f1, *pu, *pv, mask, frame, *u, *v, bag, Options(*options), &r);
    Report(report, &r, 1);
    return im.Finish(h->flow, total_ms);
}

// OpticalFlow2D::ComputeFlowSequenceWarmDevice: frame_count frames, frame_count - 1 flows; reports: frame_count - 1 entries or null.
HOST_API int flow2d_host_compute_flow_sequence_warm_device(flow2d_host_flow* h, void* const* dev_frames, size_t frame_count,
                                                           void* const* dev_flows_u, void* const* dev_flows_v,
                                                           const flow2d_host_params* params, float reach, int prior_level,
                                                           const flow2d_host_warm_options* options, flow2d_host_warm_report* reports)
{
    if (!h || !params || !options || !dev_frames || !dev_flows_u || !dev_flows_v || frame_count < 2) return 1;
    PriorBag bag(*params, reach, prior_level);
    h->flow.timing_mode = 0;
    const std::vector<DevicePtr> frames = DevicePtrs(dev_frames, frame_count), us = DevicePtrs(dev_flows_u, frame_count - 1),
                                 vs = DevicePtrs(dev_flows_v, frame_count - 1);
    std::vector<OpticalFlow2D::WarmReport> r(frame_count - 1);
    if (!h->flow.ComputeFlowSequenceWarmDevice(frames.data(), frame_count, us.data(), vs.data(), bag, Options(*options),
                                               reports ? r.data() : nullptr))
        return 2;
    Report(reports, r.data(), r.size());
    return 0;
}

// OpticalFlow2D::ComputeFlowSequenceWarm on tight host images: frames = frame_count images, flows_u / flows_v = frame_count - 1 each.
HOST_API int flow2d_host_compute_flow_sequence_warm(flow2d_host_flow* h, const float* frames, size_t frame_count, float* flows_u,
                                                    float* flows_v, const flow2d_host_params* params, float reach, int prior_level,
                                                    const flow2d_host_warm_options* options, flow2d_host_warm_report* reports,
                                                    float* total_ms)
{
    if (!h || !frames || !flows_u || !flows_v || !params || !options || frame_count < 2) return 1;
    HostImages im(h);
    Data2D* in = im.In(frames, frame_count);
    Data2D *us = im.Out(flows_u, im.Always, frame_count - 1), *vs = im.Out(flows_v, im.Always, frame_count - 1);
    const std::vector<Data2D*> frame_ptrs = Pointers(in, frame_count);
    PriorBag bag(*params, reach, prior_level);
    std::vector<OpticalFlow2D::WarmReport> r(frame_count - 1);
    h->flow.ComputeFlowSequenceWarm(frame_ptrs.data(), frame_count, us, vs, bag, Options(*options), r.data());
    Report(reports, r.data(), r.size());
    return im.Finish(h->flow, total_ms);
}

// Whether ComputeFlowBidirectional refuses a bag that carries the keys of a prior (there is no prior for the backward flow): runs it
// on two zero frames with prior_reach in the bag; 1 when no flow was delivered.
HOST_API int flow2d_host_bidirectional_refuses_prior(flow2d_host_flow* h, const flow2d_host_params* params)
{
    if (!h || !params) return -1;
    std::vector<Data2D> images;
    for (int i = 0; i < 8; ++i) images.emplace_back(h->width, h->height);
    for (size_t i = 0; i < h->width * h->height; ++i) images[0].DataPtr()[i] = images[1].DataPtr()[i] = 0.f;
    PriorBag bag(*params, 2.f, -1);
    h->flow.ComputeFlowBidirectional(images[0], images[1], images[2], images[3], images[4], images[5], images[6], images[7], bag);
    return h->flow.LastRunSucceeded() ? 0 : 1;
}

// OpticalFlow2D::StabiliseSequence on tight host images: frames = frame_count * width * height floats (frame k at k * width *
// height); outputs get the same layout, motions (optional) frame_count records.  0 on success, 1 for a null or refused argument,
// 2 when the run delivered no frames.
HOST_API int flow2d_host_stabilise_sequence(flow2d_host_flow* h, const float* frames, size_t frame_count, size_t reference_index,
                                            int model, double sigma, int iterations, int use_masks, float fill, float* outputs,
                                            flow2d_global_motion* motions, const flow2d_host_params* params, float* total_ms)
{
    if (!OpticalFlow2D::GlobalMotionArgsOk(model, sigma, iterations) || !h || !frames || !outputs || !params || frame_count < 2 ||
        reference_index >= frame_count)
        return 1;
    HostImages im(h);
    const std::vector<Data2D*> fp = Pointers(im.In(frames, frame_count), frame_count);
    Data2D* out = im.Out(outputs, im.Always, frame_count);
    Bag bag(*params);
    h->flow.StabiliseSequence(fp.data(), frame_count, reference_index, model, sigma, iterations, use_masks != 0, fill, out, motions, bag);
    return im.Finish(h->flow, total_ms);
}

// OpticalFlow2D::StabiliseSequenceDevice: frame_count device frames and output planes, motions (host, optional) frame_count
// records.  Synchronises.  0 on success, 1 for a null or refused argument.
HOST_API int flow2d_host_stabilise_sequence_device(flow2d_host_flow* h, void* const* dev_frames, size_t frame_count,
                                                   size_t reference_index, int model, double sigma, int iterations, int use_masks,
                                                   float fill, void* const* dev_outputs, flow2d_global_motion* motions,
                                                   const flow2d_host_params* params)
{
    if (!OpticalFlow2D::GlobalMotionArgsOk(model, sigma, iterations) || !h || !params || !dev_frames || !dev_outputs ||
        frame_count < 2 || reference_index >= frame_count)
        return 1;
    Bag bag(*params);
    h->flow.timing_mode = 0;
    const std::vector<DevicePtr> frames = DevicePtrs(dev_frames, frame_count), outputs = DevicePtrs(dev_outputs, frame_count);
    return h->flow.StabiliseSequenceDevice(frames.data(), frame_count, reference_index, model, sigma, iterations, use_masks != 0, fill,
                                           outputs.data(), motions, bag)
               ? 0
               : 2;
}

// OpticalFlow2D::ComputeFlowBidirectionalDevice: frame_count device frames, frame_count - 1 forward and backward flow plane pairs,
// occlusion planes optional (NULL arrays: no masks).  Queued on the context's stream, no synchronisation.  0 on success.
HOST_API int flow2d_host_compute_flow_bidirectional_device(flow2d_host_flow* h, void* const* dev_frames, size_t frame_count,
                                                           void* const* dev_flows_u, void* const* dev_flows_v,
                                                           void* const* dev_back_us, void* const* dev_back_vs,
                                                           void* const* dev_occ_fwd, void* const* dev_occ_bwd,
                                                           const flow2d_host_params* params, float alpha1, float alpha2)
{
    if (!h || !params || !dev_frames || !dev_flows_u || !dev_flows_v || !dev_back_us || !dev_back_vs || frame_count < 2)
        return 1;
    Bag bag(*params, alpha1, alpha2);
    h->flow.timing_mode = 0;
    const std::vector<DevicePtr> frames = DevicePtrs(dev_frames, frame_count);
    void* const* sources[6] = {dev_flows_u, dev_flows_v, dev_back_us, dev_back_vs, dev_occ_fwd, dev_occ_bwd};
    std::vector<DevicePtr> planes[6];
    for (int i = 0; i < 6; ++i) planes[i] = DevicePtrs(sources[i], frame_count - 1);
    auto arr = [&](int i) { return sources[i] ? planes[i].data() : nullptr; };
    return h->flow.ComputeFlowBidirectionalDevice(frames.data(), frame_count, arr(0), arr(1), arr(2), arr(3), arr(4), arr(5), bag)
               ? 0
               : 2;
}

// ---- OpticalFlowBatch2D: pairs spread over lanes (stream + OpticalFlow2D + plane pool each) on one GPU -----------
struct flow2d_host_batch {
    OpticalFlowBatch2D batch;
};

HOST_API flow2d_host_batch* flow2d_host_batch_create(size_t width, size_t height, int constancy, size_t lanes, int device,
                                                     size_t group_size)
{
    flow2d_host_batch* h = new (std::nothrow) flow2d_host_batch();
    if (!h) return nullptr;
    DataSize3 size = {width, height, 1};
    if (!h->batch.Initialize(size, static_cast<DataConstancy>(constancy), lanes, device, group_size)) {
        delete h;
        return nullptr;
    }
    return h;
}

HOST_API void flow2d_host_batch_destroy(flow2d_host_batch* h)
{
    if (!h) return;
    h->batch.Destroy();
    delete h;
}

HOST_API size_t flow2d_host_batch_pitch(flow2d_host_batch* h) { return h ? h->batch.ContainerSize().pitch : 0; }
HOST_API size_t flow2d_host_batch_lanes(flow2d_host_batch* h) { return h ? h->batch.Lanes() : 0; }
HOST_API size_t flow2d_host_batch_group_stride(flow2d_host_batch* h) { return h ? h->batch.GroupStrideBytes() : 0; }
HOST_API flow2d_context* flow2d_host_batch_lane_context(flow2d_host_batch* h, size_t lane)
{
    return h ? h->batch.LaneContext(lane) : nullptr;
}
HOST_API void flow2d_host_batch_use_graph(flow2d_host_batch* h, int on)
{
    if (h) h->batch.use_graph = on != 0;
}

// OpticalFlowBatch2D::ComputeFlowBatchDevice: `count` pairs, pair k on lane (first_lane + k) mod lanes.  0 on success.
HOST_API int flow2d_host_batch_compute(flow2d_host_batch* h, size_t count, void* const* dev_frames_0,
                                       void* const* dev_frames_1, void* const* dev_flows_u, void* const* dev_flows_v,
                                       const flow2d_host_params* params, size_t first_lane)
{
    if (!h || !params || (count && (!dev_frames_0 || !dev_frames_1 || !dev_flows_u || !dev_flows_v))) return 1;
    Bag bag(*params);
    const std::vector<DevicePtr> f0 = DevicePtrs(dev_frames_0, count), f1 = DevicePtrs(dev_frames_1, count),
                                 u = DevicePtrs(dev_flows_u, count), v = DevicePtrs(dev_flows_v, count);
    return h->batch.ComputeFlowBatchDevice(count, f0.data(), f1.data(), u.data(), v.data(), bag, first_lane) ? 0 : 2;
}

// OpticalFlowBatch2D::ComputeFlowBatchDeviceGrouped: `count` independent pairs, grouped by the object.  0 on success.
HOST_API int flow2d_host_batch_compute_grouped(flow2d_host_batch* h, size_t count, void* const* dev_frames_0,
                                               void* const* dev_frames_1, void* const* dev_flows_u,
                                               void* const* dev_flows_v, const flow2d_host_params* params,
                                               size_t first_lane)
{
    if (!h || !params || (count && (!dev_frames_0 || !dev_frames_1 || !dev_flows_u || !dev_flows_v))) return 1;
    Bag bag(*params);
    const std::vector<DevicePtr> f0 = DevicePtrs(dev_frames_0, count), f1 = DevicePtrs(dev_frames_1, count),
                                 u = DevicePtrs(dev_flows_u, count), v = DevicePtrs(dev_flows_v, count);
    return h->batch.ComputeFlowBatchDeviceGrouped(count, f0.data(), f1.data(), u.data(), v.data(), bag, first_lane) ? 0 : 2;
}

// Host images for the H<->D-inclusive entry: Data2D objects in pageable or page-locked memory (HostMemory::Pinned, the
// reference's ALLOCATE_PINNED_MEMORY option as a run-time choice).  The caller fills / reads them through the pointer.
HOST_API Data2D* flow2d_host_data2d_create(size_t width, size_t height, int pinned)
{
    Data2D* d = new (std::nothrow) Data2D(width, height, pinned ? HostMemory::Pinned : HostMemory::Pageable);
    if (d && !d->DataPtr()) {
        delete d;
        d = nullptr;
    }
    return d;
}
HOST_API void flow2d_host_data2d_destroy(Data2D* d) { delete d; }
HOST_API void flow2d_host_use_pinned_memory(int on) { Data2D::UsePinnedMemory(on != 0); }
HOST_API float* flow2d_host_data2d_ptr(Data2D* d) { return d ? d->DataPtr() : nullptr; }
HOST_API int flow2d_host_data2d_is_pinned(Data2D* d) { return d && d->IsPinned() ? 1 : 0; }

// OpticalFlowBatch2D::ComputeFlowBatch: `count` pairs of host images in, host flows out, uploads and downloads
// pipelined against the lanes' pyramids.  Queued: the flows are complete after flow2d_host_batch_synchronize.
HOST_API int flow2d_host_batch_compute_host(flow2d_host_batch* h, size_t count, Data2D* const* frames_0,
                                            Data2D* const* frames_1, Data2D* const* flows_u, Data2D* const* flows_v,
                                            const flow2d_host_params* params, size_t first_lane)
{
    if (!h || !params) return 1;
    Bag bag(*params);
    return h->batch.ComputeFlowBatch(count, frames_0, frames_1, flows_u, flows_v, bag, first_lane) ? 0 : 2;
}

HOST_API int flow2d_host_batch_synchronize(flow2d_host_batch* h) { return (h && h->batch.Synchronize()) ? 0 : 1; }

// Per-level solve records of the last run (needs timing_mode >= 1 and a synchronised context).
// Writes up to `capacity` records of 7 floats (width, height, solve_ms, kernel_ms, kernel_launches,
// algorithmic bytes per launch, algorithm used) and returns the number of levels.
HOST_API size_t flow2d_host_level_timings(flow2d_host_flow* h, float* records, size_t capacity)
{
    if (!h) return 0;
    std::vector<FlowLevelTiming> t = h->flow.LastLevelTimings();
    for (size_t i = 0; i < t.size() && i < capacity; ++i) {
        records[7 * i + 0] = static_cast<float>(t[i].width);
        records[7 * i + 1] = static_cast<float>(t[i].height);
        records[7 * i + 2] = t[i].solve_ms;
        records[7 * i + 3] = t[i].kernel_ms;
        records[7 * i + 4] = static_cast<float>(t[i].kernel_launches);
        records[7 * i + 5] = static_cast<float>(t[i].bytes_per_launch);
        records[7 * i + 6] = static_cast<float>(t[i].algorithm);
    }
    return t.size();
}

HOST_API void flow2d_host_use_graph(flow2d_host_flow* h, int on)
{
    if (h) h->flow.use_graph = on != 0;
}

HOST_API void flow2d_host_reset_timings(flow2d_host_flow* h)
{
    if (h) h->flow.ResetLevelTimings();
}

// Omitting a bag key must make ComputeFlow print and return with the outputs untouched
// (optical_flow_2d.cpp:160-168).  Returns 1 if the outputs were left untouched.
HOST_API int flow2d_host_missing_key_leaves_outputs(flow2d_host_flow* h, const char* omitted_key)
{
    if (!h) return -1;
    Data2D f0(h->width, h->height), f1(h->width, h->height), u(h->width, h->height), v(h->width, h->height);
    const size_t n = h->width * h->height;
    for (size_t i = 0; i < n; ++i) u.DataPtr()[i] = v.DataPtr()[i] = 77.f;
    Bag full(flow2d_host_params{3, 0.5f, 1, 1, 3.5f, 0.001f, 0.001f, 5, 0.45f, 0, 0.f});
    OperationParameters bag;
    const char* keys[] = {"warp_levels_count", "warp_scale_factor", "outer_iterations_count",
                          "inner_iterations_count", "equation_alpha", "equation_smoothness",
                          "equation_data", "median_radius", "gaussian_sigma"};
    for (const char* k : keys)
        if (std::strcmp(k, omitted_key) != 0) bag.PushValuePtr(k, full.bag.GetValuePtr(k));
    h->flow.ComputeFlow(f0, f1, u, v, bag);
    for (size_t i = 0; i < n; ++i)
        if (u.DataPtr()[i] != 77.f || v.DataPtr()[i] != 77.f) return 0;
    return 1;
}

// ---- small helpers so the tests can reach Data2D / Settings / IOUtils ---------------------------------
HOST_API int flow2d_host_read_raw(const char* path, size_t width, size_t height, int u8, float* out)
{
    Data2D d;
    const bool ok = u8 ? d.ReadRAWFromFileU8(path, width, height) : d.ReadRAWFromFileF32(path, width, height);
    if (!ok) return 1;
    std::memcpy(out, d.DataPtr(), width * height * sizeof(float));
    return 0;
}

// Data2D::WriteRAWToFileU8 / WriteRAWToFileF32 of a tight width x height image.  0 on success.
HOST_API int flow2d_host_write_raw(const float* data, size_t width, size_t height, int u8, const char* path)
{
    Data2D d(width, height);
    std::memcpy(d.DataPtr(), data, width * height * sizeof(float));
    return (u8 ? d.WriteRAWToFileU8(path) : d.WriteRAWToFileF32(path)) ? 0 : 1;
}

// IOUtils::ReadFlowFLO: *width / *height get the file's size; the flow goes to u / v (width * height floats each) when both are
// given and capacity (in floats) holds it -- call with u = v = NULL first to learn the size.  0 on success, 1 when the file is
// refused, 2 when the buffers are too small.
HOST_API int flow2d_host_read_flo(const char* path, size_t* width, size_t* height, float* u, float* v, size_t capacity)
{
    if (!path || !width || !height) return 1;
    Data2D du, dv;
    if (!IOUtils::ReadFlowFLO(path, du, dv)) return 1;
    *width = du.Width();
    *height = du.Height();
    const size_t n = du.Width() * du.Height();
    if (!u && !v) return 0;
    if (!u || !v || capacity < n) return 2;
    std::memcpy(u, du.DataPtr(), n * sizeof(float));
    std::memcpy(v, dv.DataPtr(), n * sizeof(float));
    return 0;
}

// IOUtils::WriteFlowFLO of tight width x height planes.  0 on success.
HOST_API int flow2d_host_write_flo(const float* u, const float* v, size_t width, size_t height, const char* path)
{
    if (!u || !v || !path || width == 0 || height == 0) return 1;
    Data2D du(width, height), dv(width, height);
    std::memcpy(du.DataPtr(), u, width * height * sizeof(float));
    std::memcpy(dv.DataPtr(), v, width * height * sizeof(float));
    return IOUtils::WriteFlowFLO(du, dv, path) ? 0 : 1;
}

// EvaluateFlow on tight host planes (occlusion, epe and ae may be NULL) on the process-wide context: the record into *out.
// 0 on success, 1 for a bad argument, 2 when there is no context or a device call failed.
HOST_API int flow2d_host_flow_error(const float* u, const float* v, const float* gt_u, const float* gt_v, const float* occlusion,
                                    size_t width, size_t height, float* epe, float* ae, flow2d_flow_error_stats* out)
{
    if (!u || !v || !gt_u || !gt_v || !out || width == 0 || height == 0) return 1;
    const size_t n = width * height;
    Data2D planes[5];
    const float* sources[5] = {u, v, gt_u, gt_v, occlusion};
    for (int i = 0; i < 5; ++i) {
        if (!sources[i]) continue;
        planes[i] = Data2D(width, height);
        std::memcpy(planes[i].DataPtr(), sources[i], n * sizeof(float));
    }
    Data2D de, da;
    if (!EvaluateFlow(planes[0], planes[1], planes[2], planes[3], occlusion ? &planes[4] : nullptr, *out, epe ? &de : nullptr,
                      ae ? &da : nullptr))
        return 2;
    if (epe) std::memcpy(epe, de.DataPtr(), n * sizeof(float));
    if (ae) std::memcpy(ae, da.DataPtr(), n * sizeof(float));
    return 0;
}

HOST_API int flow2d_host_write_outputs(const float* u, const float* v, size_t width, size_t height,
                                       const char* ppm_path, const char* amp_path, float flow_max_scale)
{
    Data2D du(width, height), dv(width, height);
    std::memcpy(du.DataPtr(), u, width * height * sizeof(float));
    std::memcpy(dv.DataPtr(), v, width * height * sizeof(float));
    IOUtils::WriteFlowToImageRGB(du, dv, flow_max_scale, ppm_path);
    IOUtils::WriteMagnitudeToFileF32(du, dv, amp_path);
    return 0;
}

HOST_API void flow2d_host_convert_to_rgb(float x, float y, int* rgb)
{
    const IOUtils::RGBColor c = IOUtils::ConvertToRGB(x, y);
    rgb[0] = c.r;
    rgb[1] = c.g;
    rgb[2] = c.b;
}

struct flow2d_host_settings {
    int width, height, medianRadius, iterInner, iterOuter, levels, press_key;
    float sigma, alpha, e_smooth, e_data, warpScale;
    char inputPath[512], outputPath[512], fileName1[256], fileName2[256], imageType[32], dataConstancy[32];
};

HOST_API int flow2d_host_load_settings(const char* path, flow2d_host_settings* out)
{
    OpticFlow::Settings s;
    const int rc = s.LoadSettings(path);
    if (rc != 0) return rc;
    out->width = s.width;
    out->height = s.height;
    out->medianRadius = s.medianRadius;
    out->iterInner = s.iterInner;
    out->iterOuter = s.iterOuter;
    out->levels = s.levels;
    out->press_key = s.press_key;
    out->sigma = s.sigma;
    out->alpha = s.alpha;
    out->e_smooth = s.e_smooth;
    out->e_data = s.e_data;
    out->warpScale = s.warpScale;
    std::snprintf(out->inputPath, sizeof(out->inputPath), "%s", s.inputPath.c_str());
    std::snprintf(out->outputPath, sizeof(out->outputPath), "%s", s.outputPath.c_str());
    std::snprintf(out->fileName1, sizeof(out->fileName1), "%s", s.fileName1.c_str());
    std::snprintf(out->fileName2, sizeof(out->fileName2), "%s", s.fileName2.c_str());
    std::snprintf(out->imageType, sizeof(out->imageType), "%s", s.imageType.c_str());
    std::snprintf(out->dataConstancy, sizeof(out->dataConstancy), "%s", s.dataConstancy.c_str());
    return 0;
}

// ---- operator-level access: the reference's plugin API (CudaOperationBase::Initialize / Execute with a
// string-keyed bag of void*) driven from the tests.  `kind`: add, convolution, median, registration, resample,
// solve.  The bag is given as parallel arrays of keys and pointers to the values (exactly what PushValuePtr takes).
#include <memory>
#include <string>

struct flow2d_host_operator {
    std::unique_ptr<CudaOperationBase> op;
    DataSize3 container;
    DataConstancy constancy;
    flow2d_context* ctx;
};

HOST_API flow2d_host_operator* flow2d_host_operator_create(const char* kind, size_t container_width,
                                                           size_t container_height, size_t pitch_bytes, int constancy,
                                                           int omit_container_size)
{
    auto h = std::make_unique<flow2d_host_operator>();
    const std::string k = kind ? kind : "";
    if (k == "add") h->op.reset(new CudaOperationAdd2D());
    else if (k == "convolution") h->op.reset(new CudaOperationConvolution2D());
    else if (k == "median") h->op.reset(new CudaOperationMedian2D());
    else if (k == "registration") h->op.reset(new CudaOperationRegistration2D());
    else if (k == "resample") h->op.reset(new CudaOperationResample2D());
    else if (k == "solve") h->op.reset(new CudaOperationSolve2D());
    else return nullptr;
    h->container = {container_width, container_height, pitch_bytes};
    h->constancy = static_cast<DataConstancy>(constancy);
    h->ctx = CurrentDeviceContext();
    OperationParameters init;
    if (!omit_container_size) init.PushValuePtr("container_size", &h->container);
    init.PushValuePtr("data_constancy", &h->constancy);
    if (!h->op->Initialize(&init)) return nullptr;
    return h.release();
}

HOST_API const char* flow2d_host_operator_name(flow2d_host_operator* h) { return h ? h->op->GetName() : ""; }

HOST_API void flow2d_host_operator_execute(flow2d_host_operator* h, const char* const* keys, void* const* values,
                                           size_t count)
{
    if (!h) return;
    OperationParameters bag;
    for (size_t i = 0; i < count; ++i) bag.PushValuePtr(keys[i], values[i]);
    h->op->Execute(bag);
}

HOST_API void flow2d_host_operator_destroy(flow2d_host_operator* h)
{
    if (!h) return;
    h->op->Destroy();
    delete h;
}

// OperationParameters semantics (operation_parameters.cpp:28-47): no overwrite, nullptr for a missing key.
HOST_API int flow2d_host_bag_selftest(void)
{
    OperationParameters bag;
    int a = 1, b = 2;
    if (!bag.PushValuePtr("k", &a)) return 1;
    if (bag.PushValuePtr("k", &b)) return 2;            // an existing key is kept
    if (bag.GetValuePtr("k") != &a) return 3;
    if (bag.GetValuePtr("missing") != nullptr) return 4;
    bag.Clear();
    if (bag.GetValuePtr("k") != nullptr) return 5;
    return 0;
}
