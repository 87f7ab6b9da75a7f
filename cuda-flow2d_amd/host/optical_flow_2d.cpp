#include "optical_flow_2d.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "device_utils.h"

namespace {
// The frame of a host-image entry.  From its construction to its destruction: the start line, two events around the uploads,
// the device work and the downloads, the entry's one host wait (on the second event), the total printed and left in
// `total_ms`.  An entry that allocated planes for this call alone names them in `per_call`: the stream is then drained and
// they are freed (the arrays must outlive the scope).
struct PlaneList {
    const DevicePtr* planes;
    size_t count;
};

class HostCall {
public:
    HostCall(flow2d_context* context, float& total_ms, PlaneList a = {nullptr, 0}, PlaneList b = {nullptr, 0},
             PlaneList c = {nullptr, 0})
        : context_(context), total_ms_(total_ms), per_call_{a, b, c}
    {
        std::printf("\nStarting optical flow computation...\n");
        flow2d_event_create(context_, &start_);
        flow2d_event_create(context_, &stop_);
        flow2d_event_record(context_, start_);
    }
    ~HostCall()
    {
        flow2d_event_record(context_, stop_);
        flow2d_event_synchronize(context_, stop_);
        flow2d_event_elapsed_ms(context_, start_, stop_, &total_ms_);
        std::printf("Total GPU computation time: % 4.4fs\n", total_ms_ / 1000.);
        flow2d_event_destroy(context_, start_);
        flow2d_event_destroy(context_, stop_);
        if (!per_call_[0].planes) return;
        flow2d_synchronize(context_);
        for (const PlaneList& list : per_call_)
            for (size_t i = 0; i < list.count; ++i)
                if (list.planes[i]) flow2d_plane_free(context_, AsPlane(list.planes[i]));
    }
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;

private:
    flow2d_context* context_;
    float& total_ms_;
    PlaneList per_call_[3];
    void *start_ = nullptr, *stop_ = nullptr;
};

// Whether every image has the initialised size (a null entry does not); prints the entries' message otherwise.
struct SizeCheck {
    DataSize3 size;
    const char *name, *what;

    bool operator()(Data2D* const* images, size_t count) const
    {
        for (size_t i = 0; i < count; ++i)
            if (!images[i] || images[i]->Width() != size.width || images[i]->Height() != size.height) {
                std::printf("Error: '%s': %s sizes do not match the initialised size %zu x %zu.\n", name, what, size.width,
                            size.height);
                return false;
            }
        return true;
    }
    bool operator()(Data2D* images, size_t count) const  // an array of images
    {
        for (size_t i = 0; i < count; ++i) {
            Data2D* one = images + i;
            if (!(*this)(&one, 1)) return false;
        }
        return true;
    }
};
}  // namespace

// ---- base ------------------------------------------------------------------------------------------
size_t OpticalFlowBase2D::GetMaxWarpLevel(size_t width, size_t height, float scale_factor) const
{
    // Level n is usable while ceil(W * s^n) >= 4 and ceil(H * s^n) >= 4, all in float
    // (optical_flow_base_2d.cpp:36-59).
    size_t level_w = 1, level_h = 1, levels = 1;
    for (; scale_factor < 1.f; ++levels) {
        const float s = std::pow(scale_factor, static_cast<float>(levels));
        level_w = static_cast<size_t>(std::ceil(width * s));
        level_h = static_cast<size_t>(std::ceil(height * s));
        if (level_w < 4 || level_h < 4) break;
    }
    if (level_w == 1 || level_h == 1) --levels;
    return levels;
}

bool OpticalFlowBase2D::IsInitialized() const
{
    if (!initialized_) std::printf("Error: '%s' was not initialized.\n", name_);
    return initialized_;
}

void OpticalFlowBase2D::ComputeFlow(Data2D&, Data2D&, Data2D&, Data2D&, OperationParameters&)
{
    std::printf("Warning: '%s' ComputeFlow() was not defined.\n", name_);
}

void OpticalFlowBase2D::Destroy() { initialized_ = false; }

OpticalFlowBase2D::~OpticalFlowBase2D() = default;

// ---- OpticalFlow2D ---------------------------------------------------------------------------------
OpticalFlow2D::OpticalFlow2D() : OpticalFlowBase2D("Optical Flow 2D MI355X") {}

OpticalFlow2D::~OpticalFlow2D() { Destroy(); }

bool OpticalFlow2D::Initialize(const DataSize3& data_size, DataConstancy data_constancy)
{
    if (initialized_) Destroy();
    context_ = CurrentDeviceContext();
    if (!context_) {
        std::printf("Error: '%s': no device context, call InitDeviceContext() first.\n", GetName());
        return false;
    }
    if (data_size.width < 4 || data_size.height < 4) {
        std::printf("Error: '%s': frames must be at least 4 x 4.\n", GetName());
        return false;
    }
    if (group_size == 0 || group_size > 64) {
        std::printf("Error: '%s': group size %zu (1..64).\n", GetName(), group_size);
        return false;
    }
    group_ = group_size;
    (void)flow2d_context_set_lone(context_, lone ? 1 : 0);
    dev_container_size_ = data_size;
    dev_container_size_.pitch = 0;
    data_constancy_ = data_constancy;
    initialized_ = InitMemory() && InitOperations();
    if (!initialized_) Destroy();
    return initialized_;
}

bool OpticalFlow2D::InitMemory()
{
    if (!silent) std::printf("Allocating memory on the device...\n");
    size_t free_bytes = 0, total_bytes = 0;
    if (CheckFlow2DError(flow2d_mem_info(context_, &free_bytes, &total_bytes), "flow2d_mem_info")) return false;
    const size_t pitch = flow2d_plane_pitch_bytes(dev_container_size_.width);
    // (+ the two packed x-pass planes; a lock-step group holds every plane group_ containers tall)
    const size_t needed = pitch * dev_container_size_.height * group_ * (kContainersCount + 3);
    if (!silent)
        std::printf("Available\t:\t%.0fMB / %.0fMB\nNeeded\t\t:\t%.0fMB\n", free_bytes / 1048576.f,
                    total_bytes / 1048576.f, needed / 1048576.f);
    if (needed >= free_bytes) return false;  // same silent refusal as optical_flow_2d.cpp:109-113
    for (size_t i = 0; i < kContainersCount; ++i) {
        void* plane = nullptr;
        size_t got_pitch = 0;
        if (CheckFlow2DError(flow2d_plane_alloc(context_, dev_container_size_.width, dev_container_size_.height * group_,
                                                &plane, &got_pitch),
                             "flow2d_plane_alloc") ||
            got_pitch != pitch) {
            std::printf("Error during device memory allocation.");
            return false;
        }
        all_planes_.push_back(static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane)));
    }
    free_planes_ = all_planes_;
    for (DevicePtr& packed : packed_frames_) {  // outside the pool: they hold one pair's x-resampled rows of all levels
        void* plane = nullptr;
        size_t got_pitch = 0;
        if (CheckFlow2DError(flow2d_plane_alloc(context_, dev_container_size_.width, dev_container_size_.height * group_,
                                                &plane, &got_pitch),
                             "flow2d_plane_alloc") ||
            got_pitch != pitch) {
            std::printf("Error during device memory allocation.");
            return false;
        }
        packed = static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane));
    }
    {  // ... and the plane the warp writes when the levels are stacked (RunPyramid); without it the levels are resampled one by one
        void* plane = nullptr;
        size_t got_pitch = 0;
        if (flow2d_plane_alloc(context_, dev_container_size_.width, dev_container_size_.height * group_, &plane, &got_pitch) == FLOW2D_OK) {
            if (got_pitch == pitch) level_warp_plane_ = static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane));
            else flow2d_plane_free(context_, plane);
        }
    }
    dev_container_size_.pitch = pitch;
    return true;
}

bool OpticalFlow2D::InitOperations()
{
    if (dev_container_size_.pitch == 0) {
        std::printf("Initialization failed. Device pitch is 0.\n");
        return false;
    }
    OperationParameters op;
    op.PushValuePtr("container_size", &dev_container_size_);
    op.PushValuePtr("data_constancy", &data_constancy_);
    op.PushValuePtr("flow2d_context", &context_);
    CudaOperationBase* ops[] = {&cuop_add_, &cuop_convolution_, &cuop_median_,
                                &cuop_register_, &cuop_resample_, &cuop_solve_};
    for (CudaOperationBase* cuop : ops) {
        const bool ok = cuop->Initialize(&op);
        if (!silent) std::printf("%-18s: %s\n", cuop->GetName(), ok ? "OK" : "FAILED");
        if (!ok) return false;
    }
    return true;
}

void OpticalFlow2D::Destroy()
{
    CudaOperationBase* ops[] = {&cuop_add_, &cuop_convolution_, &cuop_median_,
                                &cuop_register_, &cuop_resample_, &cuop_solve_};
    for (CudaOperationBase* cuop : ops) cuop->Destroy();
    if (context_) {
        if (!all_planes_.empty()) flow2d_synchronize(context_);
        DropGraphs();
        FreeSequenceCache();
        if (free_planes_.size() != all_planes_.size())
            std::printf("Warning. Not all device memory allocations were freed.\n");
        for (DevicePtr p : all_planes_) flow2d_plane_free(context_, AsPlane(p));
        for (DevicePtr& p : packed_frames_) {
            if (p) flow2d_plane_free(context_, AsPlane(p));
            p = 0;
        }
        for (DevicePtr& p : group_staging_) {
            if (p) flow2d_plane_free(context_, AsPlane(p));
            p = 0;
        }
        if (level_warp_plane_) flow2d_plane_free(context_, AsPlane(level_warp_plane_));
        level_warp_plane_ = 0;
        for (DevicePtr& p : bidirectional_planes_) {
            if (p) flow2d_plane_free(context_, AsPlane(p));
            p = 0;
        }
        for (DevicePtr& p : interpolation_planes_) {
            if (p) flow2d_plane_free(context_, AsPlane(p));
            p = 0;
        }
        for (DevicePtr p : interpolation_outputs_) flow2d_plane_free(context_, AsPlane(p));
        interpolation_outputs_.clear();
        for (DevicePtr p : tracking_flows_) flow2d_plane_free(context_, AsPlane(p));
        tracking_flows_.clear();
        if (tracking_scratch_) flow2d_plane_free(context_, AsPlane(tracking_scratch_));
        tracking_scratch_ = 0;
        tracking_scratch_bytes_ = 0;
        if (stabilise_scratch_) flow2d_plane_free(context_, AsPlane(stabilise_scratch_));
        stabilise_scratch_ = 0;
        if (segment_scratch_) flow2d_plane_free(context_, AsPlane(segment_scratch_));
        segment_scratch_ = 0;
        for (DevicePtr& p : segment_planes_) {
            if (p) flow2d_plane_free(context_, AsPlane(p));
            p = 0;
        }
        if (deformation_scratch_) flow2d_plane_free(context_, AsPlane(deformation_scratch_));
        deformation_scratch_ = 0;
        for (DevicePtr& p : deformation_planes_) {
            if (p) flow2d_plane_free(context_, AsPlane(p));
            p = 0;
        }
        for (std::vector<DevicePtr>* planes : {&denoise_pairs_, &denoise_chains_, &stabilise_planes_}) {
            for (DevicePtr p : *planes)
                if (p) flow2d_plane_free(context_, AsPlane(p));
            planes->clear();
        }
    }
    all_planes_.clear();
    free_planes_.clear();
    initialized_ = false;
}

DevicePtr OpticalFlow2D::Acquire()
{
    DevicePtr p = free_planes_.back();
    free_planes_.pop_back();
    return p;
}

void OpticalFlow2D::Release(DevicePtr p) { free_planes_.push_back(p); }

void OpticalFlow2D::FreeSequenceCache()
{
    for (FramePyramid& pyramid : sequence_cache_) {
        if (context_) {
            if (pyramid.blurred) flow2d_plane_free(context_, AsPlane(pyramid.blurred));
            for (DevicePtr p : pyramid.levels)
                if (p) flow2d_plane_free(context_, AsPlane(p));
        }
        pyramid = FramePyramid();
    }
}

// The plane of `pyramid` that holds pyramid level `level` (>= 1): container width, `rows` rows, same pitch as the
// 12 containers.  Allocated on first use and whenever a later call needs more rows.  0 on failure.
DevicePtr OpticalFlow2D::SequenceLevelPlane(FramePyramid& pyramid, size_t level, size_t rows)
{
    if (pyramid.levels.size() <= level) {
        pyramid.levels.resize(level + 1, 0);
        pyramid.level_rows.resize(level + 1, 0);
    }
    if (pyramid.levels[level] && pyramid.level_rows[level] >= rows) return pyramid.levels[level];
    if (pyramid.levels[level]) {
        flow2d_synchronize(context_);  // the old plane may still be read by queued work
        flow2d_plane_free(context_, AsPlane(pyramid.levels[level]));
        pyramid.levels[level] = 0;
    }
    void* plane = nullptr;
    size_t pitch = 0;
    if (CheckFlow2DError(flow2d_plane_alloc(context_, dev_container_size_.width, rows, &plane, &pitch), "flow2d_plane_alloc"))
        return 0;
    if (pitch != dev_container_size_.pitch) {
        flow2d_plane_free(context_, static_cast<float*>(plane));
        std::printf("Error: '%s': sequence cache pitch %zu differs from the container pitch %zu.\n", GetName(), pitch,
                    dev_container_size_.pitch);
        return 0;
    }
    pyramid.levels[level] = static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane));
    pyramid.level_rows[level] = rows;
    return pyramid.levels[level];
}

// Every pyramid of the sequence cache invalid (the frames may have changed since the last call); a plane for the blurred
// frame when there is a pre-blur.
bool OpticalFlow2D::PrepareSequenceCache(OperationParameters& params)
{
    float gaussian_sigma = 0.f;
    params.Read<float>("gaussian_sigma", gaussian_sigma);
    for (FramePyramid& pyramid : sequence_cache_) {
        pyramid.valid = false;
        if (gaussian_sigma > 0.f && !pyramid.blurred) {  // a plane for the blurred frame
            void* plane = nullptr;
            size_t pitch = 0;
            if (CheckFlow2DError(flow2d_plane_alloc(context_, dev_container_size_.width, dev_container_size_.height,
                                                    &plane, &pitch),
                                 "flow2d_plane_alloc") ||
                pitch != dev_container_size_.pitch)
                return false;
            pyramid.blurred = static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane));
        }
    }
    return true;
}

bool OpticalFlow2D::RunSequencePair(FramePyramid& first, FramePyramid& second, DevicePtr frame_0, DevicePtr frame_1,
                                    DevicePtr flow_u, DevicePtr flow_v, OperationParameters& params)
{
    sequence_frames_[0] = &first;
    sequence_frames_[1] = &second;
    dev_frame_0_ = Acquire();  // unused by a sequence pair, kept for the pool's bookkeeping
    dev_frame_1_ = Acquire();
    dev_flow_u_ = Acquire();
    dev_flow_v_ = Acquire();
    caller_frame_0_ = frame_0;
    caller_frame_1_ = frame_1;
    caller_flow_u_ = flow_u;
    caller_flow_v_ = flow_v;
    const bool ok = RunPyramid(params);
    caller_frame_0_ = caller_frame_1_ = caller_flow_u_ = caller_flow_v_ = 0;
    sequence_frames_[0] = sequence_frames_[1] = nullptr;
    Release(dev_frame_0_);
    Release(dev_frame_1_);
    Release(dev_flow_u_);
    Release(dev_flow_v_);
    if (ok) first.valid = second.valid = true;
    return ok;
}

bool OpticalFlow2D::ComputeFlowSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, const DevicePtr* dev_flows_u,
                                              const DevicePtr* dev_flows_v, OperationParameters& params)
{
    if (!IsInitialized() || !dev_frames || !dev_flows_u || !dev_flows_v || frame_count < 2) return false;
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return false;
    }
    for (size_t k = 0; k < frame_count; ++k)
        if (!dev_frames[k] || (k + 1 < frame_count && (!dev_flows_u[k] || !dev_flows_v[k]))) return false;
    if (!PrepareSequenceCache(params)) return false;
    bool ok = true;
    for (size_t k = 0; ok && k + 1 < frame_count; ++k) {
        FramePyramid& first = sequence_cache_[k % 2];          // frame k: built as the second frame of pair k-1
        FramePyramid& second = sequence_cache_[(k + 1) % 2];   // frame k+1: built by this pair
        second.valid = false;
        ok = RunSequencePair(first, second, dev_frames[k], dev_frames[k + 1], dev_flows_u[k], dev_flows_v[k], params);
    }
    return ok;
}

bool OpticalFlow2D::ComputeFlowBidirectionalDevice(const DevicePtr* dev_frames, size_t frame_count, const DevicePtr* dev_flows_u,
                                                   const DevicePtr* dev_flows_v, const DevicePtr* dev_back_us,
                                                   const DevicePtr* dev_back_vs, const DevicePtr* dev_occ_fwd,
                                                   const DevicePtr* dev_occ_bwd, OperationParameters& params)
{
    if (!IsInitialized() || !dev_frames || !dev_flows_u || !dev_flows_v || !dev_back_us || !dev_back_vs || frame_count < 2)
        return false;
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return false;
    }
    // every plane written must be distinct from every other one and from the frames (which are only read)
    std::vector<DevicePtr> outputs;
    for (size_t k = 0; k + 1 < frame_count; ++k) {
        for (const DevicePtr* a : {dev_flows_u, dev_flows_v, dev_back_us, dev_back_vs, dev_occ_fwd, dev_occ_bwd})
            if (a) outputs.push_back(a[k]);
    }
    for (size_t k = 0; k < frame_count; ++k)
        if (!dev_frames[k]) return false;
    for (size_t i = 0; i < outputs.size(); ++i) {
        if (!outputs[i]) return false;
        for (size_t k = 0; k < frame_count; ++k)
            if (outputs[i] == dev_frames[k]) {
                std::printf("Error: '%s': an output plane is one of the frames.\n", GetName());
                return false;
            }
        for (size_t j = i + 1; j < outputs.size(); ++j)
            if (outputs[i] == outputs[j]) {
                std::printf("Error: '%s': the output planes must be distinct.\n", GetName());
                return false;
            }
    }
    float alpha1 = 0.01f, alpha2 = 0.5f;  // Sundaram, Brox & Keutzer (ECCV 2010)
    params.Read<float>("consistency_alpha1", alpha1);
    params.Read<float>("consistency_alpha2", alpha2);
    const bool masks = dev_occ_fwd || dev_occ_bwd;
    if (masks && !(std::isfinite(alpha1) && std::isfinite(alpha2) && alpha1 >= 0.f && alpha2 >= 0.f)) {
        std::printf("Error: '%s': consistency thresholds %g / %g (finite, >= 0).\n", GetName(), alpha1, alpha2);
        return false;
    }
    if (!PrepareSequenceCache(params)) return false;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    bool ok = true;
    for (size_t k = 0; ok && k + 1 < frame_count; ++k) {
        FramePyramid& first = sequence_cache_[k % 2];          // frame k: built as the second frame of pair k-1
        FramePyramid& second = sequence_cache_[(k + 1) % 2];   // frame k+1: built by the forward run
        second.valid = false;
        ok = RunSequencePair(first, second, dev_frames[k], dev_frames[k + 1], dev_flows_u[k], dev_flows_v[k], params) &&
             RunSequencePair(second, first, dev_frames[k + 1], dev_frames[k], dev_back_us[k], dev_back_vs[k], params);
        if (ok && dev_occ_fwd)
            ok = !CheckFlow2DError(flow2d_consistency_2d(context_, AsPlane(dev_flows_u[k]), AsPlane(dev_flows_v[k]),
                                                         AsPlane(dev_back_us[k]), AsPlane(dev_back_vs[k]), W, H, pitch, alpha1,
                                                         alpha2, AsPlane(dev_occ_fwd[k])),
                                   "flow2d_consistency_2d");
        if (ok && dev_occ_bwd)
            ok = !CheckFlow2DError(flow2d_consistency_2d(context_, AsPlane(dev_back_us[k]), AsPlane(dev_back_vs[k]),
                                                         AsPlane(dev_flows_u[k]), AsPlane(dev_flows_v[k]), W, H, pitch, alpha1,
                                                         alpha2, AsPlane(dev_occ_bwd[k])),
                                   "flow2d_consistency_2d");
    }
    return ok;
}

void OpticalFlow2D::ComputeFlowBidirectional(Data2D& frame_0, Data2D& frame_1, Data2D& flow_u, Data2D& flow_v, Data2D& back_u,
                                             Data2D& back_v, Data2D& occlusion_0, Data2D& occlusion_1, OperationParameters& params)
{
    last_run_ok_ = false;
    if (!IsInitialized()) return;
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return;
    }
    const size_t H = dev_container_size_.height;
    Data2D* images[8] = {&frame_0, &frame_1, &flow_u, &flow_v, &back_u, &back_v, &occlusion_0, &occlusion_1};
    if (!SizeCheck{dev_container_size_, GetName(), "frame / flow"}(images, 8)) return;
    if (!EnsurePlanes(bidirectional_planes_, 8)) return;
    HostCall call(context_, last_total_ms_);
    const DevicePtr* d = bidirectional_planes_;  // frame 0, frame 1, u, v, back u, back v, occlusion 0, occlusion 1
    bool ok = CopyData2DtoDevice(frame_0, d[0], H, dev_container_size_.pitch) &&
              CopyData2DtoDevice(frame_1, d[1], H, dev_container_size_.pitch);
    ok = ok && ComputeFlowBidirectionalDevice(d, 2, d + 2, d + 3, d + 4, d + 5, d + 6, d + 7, params);
    for (int i = 2; ok && i < 8; ++i) ok = CopyData2DFromDevice(d[i], *images[i], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::EnsurePlanes(DevicePtr* planes, size_t count)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    for (size_t i = 0; i < count; ++i) {
        if (planes[i]) continue;
        void* plane = nullptr;
        size_t pitch = 0;
        if (CheckFlow2DError(flow2d_plane_alloc(context_, W, H, &plane, &pitch), "flow2d_plane_alloc")) return false;
        planes[i] = static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane));
        if (pitch != dev_container_size_.pitch) {
            std::printf("Error: '%s': plane pitch %zu differs from the container pitch %zu.\n", GetName(), pitch,
                        dev_container_size_.pitch);
            return false;
        }
    }
    return true;
}

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
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return false;
    }
    if (!InterpolationArgsOk(times, time_count, iterations, max_residual)) return false;
    // every output must be distinct from every other one and from the frames (which are only read)
    const size_t n = (frame_count - 1) * time_count;
    for (size_t k = 0; k < frame_count; ++k)
        if (!dev_frames[k]) return false;
    for (size_t i = 0; i < n; ++i) {
        if (!dev_outputs[i]) return false;
        for (size_t k = 0; k < frame_count; ++k)
            if (dev_outputs[i] == dev_frames[k]) {
                std::printf("Error: '%s': an output plane is one of the frames.\n", GetName());
                return false;
            }
        for (size_t j = i + 1; j < n; ++j)
            if (dev_outputs[i] == dev_outputs[j]) {
                std::printf("Error: '%s': the output planes must be distinct.\n", GetName());
                return false;
            }
    }
    if (!EnsurePlanes(interpolation_planes_, 6)) return false;
    const DevicePtr* p = interpolation_planes_;  // u, v, back u, back v, occlusion 0, occlusion 1
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
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return;
    }
    if (!InterpolationArgsOk(times, time_count, iterations, max_residual)) return;
    const size_t H = dev_container_size_.height;
    Data2D* flows[6] = {flow_u, flow_v, back_u, back_v, use_masks ? occlusion_0 : nullptr, use_masks ? occlusion_1 : nullptr};
    std::vector<Data2D*> images = {&frame_0, &frame_1};
    for (size_t j = 0; j < time_count; ++j) images.push_back(outputs + j);
    for (Data2D* d : flows)
        if (d) images.push_back(d);
    if (!SizeCheck{dev_container_size_, GetName(), "frame / output"}(images.data(), images.size())) return;
    if (interpolation_outputs_.size() < time_count) interpolation_outputs_.resize(time_count, 0);
    if (!EnsurePlanes(bidirectional_planes_, 2) || !EnsurePlanes(interpolation_planes_, 6) ||
        !EnsurePlanes(interpolation_outputs_.data(), time_count))
        return;
    HostCall call(context_, last_total_ms_);
    const size_t pitch = dev_container_size_.pitch;
    const DevicePtr* f = bidirectional_planes_;  // frame 0, frame 1
    bool ok = CopyData2DtoDevice(frame_0, f[0], H, pitch) && CopyData2DtoDevice(frame_1, f[1], H, pitch) &&
              InterpolateFramesDevice(f, 2, times, time_count, interpolation_outputs_.data(), iterations, max_residual, use_masks,
                                      params);
    for (size_t j = 0; ok && j < time_count; ++j) ok = CopyData2DFromDevice(interpolation_outputs_[j], outputs[j], H, pitch);
    for (int i = 0; ok && i < 6; ++i)
        if (flows[i]) ok = CopyData2DFromDevice(interpolation_planes_[i], *flows[i], H, pitch);
    last_run_ok_ = ok;
}

// `bytes` of device memory (a one-row plane, 16-byte aligned); 0 on failure
DevicePtr OpticalFlow2D::AllocBytes(size_t bytes)
{
    void* plane = nullptr;
    size_t pitch = 0;
    if (CheckFlow2DError(flow2d_plane_alloc(context_, (bytes + 3) / 4, 1, &plane, &pitch), "flow2d_plane_alloc")) return 0;
    return static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane));
}

bool OpticalFlow2D::TrackPointsDevice(const DevicePtr* dev_frames, size_t frame_count, size_t spacing, float min_eigenvalue,
                                      bool check_boundaries, float beta1, float beta2, const DevicePtr* dev_xs,
                                      const DevicePtr* dev_ys, size_t capacity, unsigned long long* counts_out,
                                      OperationParameters& params)
{
    if (!IsInitialized() || !dev_frames || !dev_xs || !dev_ys || !counts_out || frame_count < 2 || capacity == 0) return false;
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return false;
    }
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
    std::vector<DevicePtr> tables;
    for (size_t k = 0; k < frame_count; ++k) {
        if (!dev_frames[k] || !dev_xs[k] || !dev_ys[k]) return false;
        tables.push_back(dev_xs[k]);
        tables.push_back(dev_ys[k]);
    }
    for (size_t i = 0; i < tables.size(); ++i) {
        for (size_t k = 0; k < frame_count; ++k)
            if (tables[i] == dev_frames[k]) {
                std::printf("Error: '%s': a track table is one of the frames.\n", GetName());
                return false;
            }
        for (size_t j = i + 1; j < tables.size(); ++j)
            if (tables[i] == tables[j]) {
                std::printf("Error: '%s': the track tables must be distinct.\n", GetName());
                return false;
            }
    }
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const size_t window = std::min(kTrackWindow, frame_count - 1);
    if (tracking_flows_.size() < 4 * window) tracking_flows_.resize(4 * window, 0);
    if (!EnsurePlanes(tracking_flows_.data(), 4 * window)) return false;
    // the device count (16 bytes) and the seeding workspace behind it
    const size_t workspace_bytes = flow2d_seed_points_workspace_bytes(W, H, spacing);
    if (tracking_scratch_bytes_ < 16 + workspace_bytes) {
        if (tracking_scratch_) {
            flow2d_synchronize(context_);  // queued work may still use the old one
            flow2d_plane_free(context_, AsPlane(tracking_scratch_));
        }
        tracking_scratch_bytes_ = 0;
        tracking_scratch_ = AllocBytes(16 + workspace_bytes);
        if (!tracking_scratch_) return false;
        tracking_scratch_bytes_ = 16 + workspace_bytes;
    }
    unsigned long long* dev_count = reinterpret_cast<unsigned long long*>(static_cast<uintptr_t>(tracking_scratch_));
    void* workspace = reinterpret_cast<char*>(dev_count) + 16;
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
               !CheckFlow2DError(flow2d_copy_d2h_2d(context_, counts + k, sizeof(unsigned long long), dev_count,
                                                    sizeof(unsigned long long), sizeof(unsigned long long), 1),
                                 "flow2d_copy_d2h_2d");
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
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return;
    }
    const size_t H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    if (!SizeCheck{dev_container_size_, GetName(), "frame"}(frames, frame_count)) return;
    // the frames and the tables of this call (freed at its end)
    std::vector<DevicePtr> dev_frames(frame_count, 0), dev_xs(frame_count, 0), dev_ys(frame_count, 0);
    bool ok = EnsurePlanes(dev_frames.data(), frame_count);
    for (size_t k = 0; ok && k < frame_count; ++k) ok = (dev_xs[k] = AllocBytes(capacity * 4)) && (dev_ys[k] = AllocBytes(capacity * 4));
    {
        HostCall call(context_, last_total_ms_, {dev_frames.data(), frame_count}, {dev_xs.data(), frame_count},
                      {dev_ys.data(), frame_count});
        for (size_t k = 0; ok && k < frame_count; ++k) ok = CopyData2DtoDevice(*frames[k], dev_frames[k], H, pitch);
        ok = ok && TrackPointsDevice(dev_frames.data(), frame_count, spacing, min_eigenvalue, check_boundaries, beta1, beta2,
                                     dev_xs.data(), dev_ys.data(), capacity, counts_out, params);
        const size_t table_bytes = capacity * sizeof(float);
        for (size_t k = 0; ok && k < frame_count; ++k)
            ok = !CheckFlow2DError(flow2d_copy_d2h_2d(context_, xs + k * capacity, table_bytes, AsPlane(dev_xs[k]), table_bytes,
                                                      table_bytes, 1),
                                   "flow2d_copy_d2h_2d") &&
                 !CheckFlow2DError(flow2d_copy_d2h_2d(context_, ys + k * capacity, table_bytes, AsPlane(dev_ys[k]), table_bytes,
                                                      table_bytes, 1),
                                   "flow2d_copy_d2h_2d");
    }
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
    if (stabilise_scratch_) return true;
    const size_t records = (kStabiliseWindow + 1) * sizeof(flow2d_global_motion);  // a multiple of 16
    stabilise_scratch_ = AllocBytes(records + flow2d_global_motion_workspace_bytes(dev_container_size_.width,
                                                                                   dev_container_size_.height, 1));
    return stabilise_scratch_ != 0;
}

flow2d_global_motion* OpticalFlow2D::StabiliseRecord(size_t slot) const
{
    return reinterpret_cast<flow2d_global_motion*>(static_cast<uintptr_t>(stabilise_scratch_)) + slot;
}

bool OpticalFlow2D::FitConsecutivePairs(const DevicePtr* frames, size_t count, int model, double sigma, int iterations,
                                        bool use_masks, flow2d_global_motion* records, OperationParameters& params)
{
    if (count < 2) return true;
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const size_t per_pair = use_masks ? 6 : 2;
    if (stabilise_planes_.size() < 6 * kStabiliseWindow) stabilise_planes_.resize(6 * kStabiliseWindow, 0);
    for (size_t j = 0; j < kStabiliseWindow; ++j)
        if (!EnsurePlanes(stabilise_planes_.data() + 6 * j, per_pair)) return false;
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
                 !CheckFlow2DError(flow2d_copy_d2h_2d(context_, records + start + j, sizeof(flow2d_global_motion), StabiliseRecord(j),
                                                      sizeof(flow2d_global_motion), sizeof(flow2d_global_motion), 1),
                                   "flow2d_copy_d2h_2d");
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
    if (group_ > 1) {
        std::printf("Error: '%s': global motion and lock-step groups do not combine.\n", GetName());
        return false;
    }
    if ((dev_flow_u == 0) != (dev_flow_v == 0) || (dev_residual_u == 0) != (dev_residual_v == 0)) return false;
    const DevicePtr frames[2] = {dev_frame_0, dev_frame_1};
    if (!FitConsecutivePairs(frames, 2, model, sigma, iterations, use_masks, motion_out, params)) return false;
    // the pair's flow and record are still in slot 0
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    bool ok = true;
    if (dev_flow_u) {
        const void* src[2] = {AsPlane(stabilise_planes_[0]), AsPlane(stabilise_planes_[1])};
        void* dst[2] = {AsPlane(dev_flow_u), AsPlane(dev_flow_v)};
        ok = !CheckFlow2DError(flow2d_copy_planes(context_, 2, src, dst, pitch, W, H), "flow2d_copy_planes");
    }
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
    const size_t H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    Data2D* images[6] = {&frame_0, &frame_1, flow_u, flow_v, residual_u, residual_v};
    Data2D* given[6];
    size_t given_count = 0;
    for (Data2D* d : images)
        if (d) given[given_count++] = d;
    if (!SizeCheck{dev_container_size_, GetName(), "frame / flow"}(given, given_count)) return;
    DevicePtr d[6] = {0, 0, 0, 0, 0, 0};  // the planes of this call (freed at its end)
    bool ok = EnsurePlanes(d, 6);
    {
        HostCall call(context_, last_total_ms_, {d, 6});
        ok = ok && CopyData2DtoDevice(frame_0, d[0], H, pitch) && CopyData2DtoDevice(frame_1, d[1], H, pitch);
        ok = ok && EstimateGlobalMotionDevice(d[0], d[1], model, sigma, iterations, use_masks, motion_out, params, d[2], d[3], d[4], d[5]);
        for (int i = 2; ok && i < 6; ++i)
            if (images[i]) ok = CopyData2DFromDevice(d[i], *images[i], H, pitch);
    }
    last_run_ok_ = ok;
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
    if (!segment_scratch_ && !(segment_scratch_ = AllocBytes(kTableOffset + table_bytes + workspace_bytes))) return false;
    // the flow, the fit and the residual planes (group_ > 1 is refused there); with use_masks the forward occlusion mask of
    // the pair is still in the window's slot 0 afterwards
    if (!EstimateGlobalMotionDevice(dev_frame_0, dev_frame_1, model, sigma, iterations, use_masks, motion_out, params, 0, 0,
                                    segment_planes_[0], segment_planes_[1]))
        return false;
    char* scratch = reinterpret_cast<char*>(static_cast<uintptr_t>(segment_scratch_));
    flow2d_segment_summary* summary = reinterpret_cast<flow2d_segment_summary*>(scratch);
    flow2d_motion_region* table = reinterpret_cast<flow2d_motion_region*>(scratch + kTableOffset);
    bool ok = !CheckFlow2DError(
        flow2d_segment_motion_2d(context_, AsPlane(segment_planes_[0]), AsPlane(segment_planes_[1]),
                                 use_masks ? AsPlane(stabilise_planes_[4]) : nullptr, W, H, pitch, threshold, join, min_area,
                                 reinterpret_cast<int*>(AsPlane(segment_planes_[2])), table, kSegmentMaxRegions, summary,
                                 scratch + kTableOffset + table_bytes, workspace_bytes),
        "flow2d_segment_motion_2d");
    ok = ok && !CheckFlow2DError(flow2d_copy_d2h_2d(context_, summary_out, sizeof(*summary_out), summary, sizeof(*summary_out),
                                                    sizeof(*summary_out), 1),
                                 "flow2d_copy_d2h_2d");
    if (ok && regions_out)
        ok = !CheckFlow2DError(flow2d_copy_d2h_2d(context_, regions_out, table_bytes, table, table_bytes, table_bytes, 1),
                               "flow2d_copy_d2h_2d");
    const void* src[3] = {AsPlane(segment_planes_[2]), AsPlane(segment_planes_[0]), AsPlane(segment_planes_[1])};
    void* dst[3] = {AsPlane(dev_labels), AsPlane(dev_residual_u), AsPlane(dev_residual_v)};
    if (ok && dev_labels) ok = !CheckFlow2DError(flow2d_copy_planes(context_, 1, src, dst, pitch, W, H), "flow2d_copy_planes");
    if (ok && dev_residual_u)
        ok = !CheckFlow2DError(flow2d_copy_planes(context_, 2, src + 1, dst + 1, pitch, W, H), "flow2d_copy_planes");
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
    const size_t H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    Data2D* images[5] = {&frame_0, &frame_1, labels, residual_u, residual_v};
    Data2D* given[5];
    size_t given_count = 0;
    for (Data2D* d : images)
        if (d) given[given_count++] = d;
    if (!SizeCheck{dev_container_size_, GetName(), "frame / labels / residual"}(given, given_count)) return;
    DevicePtr d[5] = {0, 0, 0, 0, 0};  // the planes of this call (freed at its end)
    bool ok = EnsurePlanes(d, 5);
    {
        HostCall call(context_, last_total_ms_, {d, 5});
        ok = ok && CopyData2DtoDevice(frame_0, d[0], H, pitch) && CopyData2DtoDevice(frame_1, d[1], H, pitch);
        ok = ok && SegmentMotionDevice(d[0], d[1], model, sigma, iterations, use_masks, threshold, join, min_area, motion_out,
                                       summary_out, regions_out, params, labels ? d[2] : 0, residual_u ? d[3] : 0,
                                       residual_u ? d[4] : 0);
        for (int i = 2; ok && i < 5; ++i)
            if (images[i]) ok = CopyData2DFromDevice(d[i], *images[i], H, pitch);
    }
    last_run_ok_ = ok;
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
    DevicePtr* p = deformation_planes_;
    if (!EnsurePlanes(p, use_masks ? 6 : 2) || (smooth && !EnsurePlanes(p + 6, 2))) return false;
    constexpr size_t kWorkspaceOffset = sizeof(flow2d_deformation_stats);  // the record comes first
    const size_t workspace_bytes = flow2d_deformation_workspace_bytes(W, H, 1);
    if (stats_out && !deformation_scratch_ && !(deformation_scratch_ = AllocBytes(kWorkspaceOffset + workspace_bytes))) return false;
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
    char* scratch = reinterpret_cast<char*>(static_cast<uintptr_t>(deformation_scratch_));
    flow2d_deformation_stats* record = stats_out ? reinterpret_cast<flow2d_deformation_stats*>(scratch) : nullptr;
    ok = ok && !CheckFlow2DError(flow2d_deformation_2d(context_, AsPlane(flow[0]), AsPlane(flow[1]), use_masks ? AsPlane(p[4]) : nullptr,
                                                       W, H, pitch, measure, &out, record,
                                                       stats_out ? scratch + kWorkspaceOffset : nullptr, workspace_bytes),
                                 "flow2d_deformation_2d");
    if (ok && stats_out)
        ok = !CheckFlow2DError(flow2d_copy_d2h_2d(context_, stats_out, sizeof(*stats_out), record, sizeof(*stats_out),
                                                  sizeof(*stats_out), 1),
                               "flow2d_copy_d2h_2d");
    const void* src[3] = {AsPlane(flow[0]), AsPlane(flow[1]), AsPlane(p[4])};
    void* dst[3] = {AsPlane(dev_flow_u), AsPlane(dev_flow_v), AsPlane(dev_mask)};
    if (ok && dev_flow_u) ok = !CheckFlow2DError(flow2d_copy_planes(context_, 2, src, dst, pitch, W, H), "flow2d_copy_planes");
    if (ok && dev_mask) ok = !CheckFlow2DError(flow2d_copy_planes(context_, 1, src + 2, dst + 2, pitch, W, H), "flow2d_copy_planes");
    return !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
}

void OpticalFlow2D::AnalyseDeformation(Data2D& frame_0, Data2D& frame_1, int measure, float smoothing_sigma, bool use_masks,
                                       Data2D* const* planes, flow2d_deformation_stats* stats_out, OperationParameters& params,
                                       Data2D* flow_u, Data2D* flow_v, Data2D* mask)
{
    last_run_ok_ = false;
    if (!DeformationArgsOk(measure, smoothing_sigma)) return;
    if (!IsInitialized() || (flow_u == nullptr) != (flow_v == nullptr) || (mask && !use_masks)) return;
    const size_t H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    Data2D* images[14] = {&frame_0, &frame_1, flow_u, flow_v, mask};
    for (int k = 0; k < 9; ++k) images[5 + k] = planes ? planes[k] : nullptr;
    Data2D* given[14];
    size_t given_count = 0;
    for (Data2D* d : images)
        if (d) given[given_count++] = d;
    if (!SizeCheck{dev_container_size_, GetName(), "frame / flow / deformation"}(given, given_count)) return;
    // the planes of this call (freed at its end): only those that are asked for
    DevicePtr d[14] = {};
    bool ok = true;
    for (int i = 0; ok && i < 14; ++i)
        if (images[i]) ok = EnsurePlanes(d + i, 1);
    {
        HostCall call(context_, last_total_ms_, {d, 14});
        ok = ok && CopyData2DtoDevice(frame_0, d[0], H, pitch) && CopyData2DtoDevice(frame_1, d[1], H, pitch);
        ok = ok && AnalyseDeformationDevice(d[0], d[1], measure, smoothing_sigma, use_masks, d + 5, stats_out, params, d[2], d[3], d[4]);
        for (int i = 2; ok && i < 14; ++i)
            if (images[i]) ok = CopyData2DFromDevice(d[i], *images[i], H, pitch);
    }
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
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return false;
    }
    for (size_t k = 0; k < frame_count; ++k) {
        if (!dev_frames[k] || !dev_outputs[k]) return false;
        for (size_t j = 0; j < frame_count; ++j)
            if (dev_outputs[k] == dev_frames[j]) {
                std::printf("Error: '%s': an output plane is one of the frames.\n", GetName());
                return false;
            }
        for (size_t j = k + 1; j < frame_count; ++j)
            if (dev_outputs[k] == dev_outputs[j]) {
                std::printf("Error: '%s': the output planes must be distinct.\n", GetName());
                return false;
            }
    }
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
            const void* src[1] = {AsPlane(dev_frames[k])};
            void* dst[1] = {AsPlane(dev_outputs[k])};
            ok = !CheckFlow2DError(flow2d_copy_planes(context_, 1, src, dst, pitch, W, H), "flow2d_copy_planes");
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
    const size_t H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const SizeCheck sizes_match{dev_container_size_, GetName(), "frame / output"};
    if (!sizes_match(frames, frame_count) || !sizes_match(outputs, frame_count)) return;
    // the frames and the outputs of this call (freed at its end)
    std::vector<DevicePtr> dev_frames(frame_count, 0), dev_outputs(frame_count, 0);
    bool ok = EnsurePlanes(dev_frames.data(), frame_count) && EnsurePlanes(dev_outputs.data(), frame_count);
    {
        HostCall call(context_, last_total_ms_, {dev_frames.data(), frame_count}, {dev_outputs.data(), frame_count});
        for (size_t k = 0; ok && k < frame_count; ++k) ok = CopyData2DtoDevice(*frames[k], dev_frames[k], H, pitch);
        ok = ok && StabiliseSequenceDevice(dev_frames.data(), frame_count, reference_index, model, sigma, iterations, use_masks,
                                           fill, dev_outputs.data(), motions_out, params);
        for (size_t k = 0; ok && k < frame_count; ++k) ok = CopyData2DFromDevice(dev_outputs[k], outputs[k], H, pitch);
    }
    last_run_ok_ = ok;
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
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return false;
    }
    // every plane written must be distinct from every other one and from the frames (which are only read)
    std::vector<DevicePtr> written(dev_outputs, dev_outputs + frame_count);
    if (dev_weight_sums) written.insert(written.end(), dev_weight_sums, dev_weight_sums + frame_count);
    for (size_t k = 0; k < frame_count; ++k)
        if (!dev_frames[k]) return false;
    for (size_t i = 0; i < written.size(); ++i) {
        if (!written[i]) return false;
        for (size_t k = 0; k < frame_count; ++k)
            if (written[i] == dev_frames[k]) {
                std::printf("Error: '%s': an output plane is one of the frames.\n", GetName());
                return false;
            }
        for (size_t j = i + 1; j < written.size(); ++j)
            if (written[i] == written[j]) {
                std::printf("Error: '%s': the output planes must be distinct.\n", GetName());
                return false;
            }
    }
    // the ring: pair j lives in slot j % slots as u, v, back u, back v, occlusion forward, occlusion backward
    const size_t slots = 2 * radius + kDenoiseWindow;
    const size_t per_slot = use_masks ? 6 : 4;
    if (denoise_pairs_.size() < 6 * slots) denoise_pairs_.resize(6 * slots, 0);
    for (size_t s = 0; s < slots; ++s)
        if (!EnsurePlanes(denoise_pairs_.data() + 6 * s, per_slot)) return false;
    // the composed flows of one centre: direction (0 backwards, 1 forwards), distance d >= 2: u, v, mask
    const size_t far = kDenoiseMaxRadius - 1;
    if (denoise_chains_.size() < 2 * far * 3) denoise_chains_.resize(2 * far * 3, 0);
    for (size_t dir = 0; dir < 2; ++dir)
        for (size_t d = 2; d <= radius; ++d)
            if (!EnsurePlanes(denoise_chains_.data() + (dir * far + d - 2) * 3, use_masks ? 3 : 2)) return false;
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
    if (group_ > 1) {
        std::printf("Error: '%s': sequences and lock-step groups do not combine.\n", GetName());
        return;
    }
    const size_t H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    const SizeCheck sizes_match{dev_container_size_, GetName(), "frame / output"};
    if (!sizes_match(frames, frame_count) || !sizes_match(outputs, frame_count) ||
        (weight_sums && !sizes_match(weight_sums, frame_count)))
        return;
    // the frames and the outputs of this call (freed at its end)
    std::vector<DevicePtr> dev_frames(frame_count, 0), dev_outputs(frame_count, 0), dev_sums(weight_sums ? frame_count : 0, 0);
    bool ok = EnsurePlanes(dev_frames.data(), frame_count) && EnsurePlanes(dev_outputs.data(), frame_count) &&
              EnsurePlanes(dev_sums.data(), dev_sums.size());
    {
        HostCall call(context_, last_total_ms_, {dev_frames.data(), frame_count}, {dev_outputs.data(), frame_count},
                      {dev_sums.data(), dev_sums.size()});
        for (size_t k = 0; ok && k < frame_count; ++k) ok = CopyData2DtoDevice(*frames[k], dev_frames[k], H, pitch);
        ok = ok && DenoiseSequenceDevice(dev_frames.data(), frame_count, radius, range_sigma, use_masks, dev_outputs.data(),
                                         weight_sums ? dev_sums.data() : nullptr, params);
        for (size_t k = 0; ok && k < frame_count; ++k) {
            ok = CopyData2DFromDevice(dev_outputs[k], outputs[k], H, pitch);
            if (ok && weight_sums) ok = CopyData2DFromDevice(dev_sums[k], weight_sums[k], H, pitch);
        }
    }
    last_run_ok_ = ok;
}

void OpticalFlow2D::ResetLevelTimings()
{
    if (context_) flow2d_timing_reset(context_);
}

std::vector<FlowLevelTiming> OpticalFlow2D::LastLevelTimings()
{
    std::vector<FlowLevelTiming> out;
    size_t n = 0;
    if (!context_ || flow2d_timing_count(context_, &n) != FLOW2D_OK) return out;
    for (size_t i = 0; i < n; ++i) {
        flow2d_timing_record r;
        if (flow2d_timing_get(context_, i, &r) != FLOW2D_OK) break;
        out.push_back({r.width, r.height, r.elapsed_ms, r.kernel_ms, r.kernel_launches, r.algorithm,
                       r.algorithmic_bytes_per_launch});
    }
    return out;
}

void OpticalFlow2D::ComputeFlow(Data2D& frame_0, Data2D& frame_1, Data2D& flow_u, Data2D& flow_v,
                                OperationParameters& params)
{
    last_run_ok_ = false;
    if (!IsInitialized()) return;
    if (group_ > 1) {
        std::printf("Error: '%s': ComputeFlow takes one pair; lock-step groups go through ComputeFlowDevice.\n", GetName());
        return;
    }
    const size_t H = dev_container_size_.height;
    Data2D* images[4] = {&frame_0, &frame_1, &flow_u, &flow_v};
    if (!SizeCheck{dev_container_size_, GetName(), "frame / flow"}(images, 4)) return;
    {
        HostCall call(context_, last_total_ms_);
        dev_frame_0_ = Acquire();
        dev_frame_1_ = Acquire();
        dev_flow_u_ = Acquire();
        dev_flow_v_ = Acquire();
        bool ok = CopyData2DtoDevice(frame_0, dev_frame_0_, H, dev_container_size_.pitch) &&
                  CopyData2DtoDevice(frame_1, dev_frame_1_, H, dev_container_size_.pitch);
        ok = ok && RunPyramid(params);
        if (ok) {
            ok = CopyData2DFromDevice(dev_flow_u_, flow_u, H, dev_container_size_.pitch) &&
                 CopyData2DFromDevice(dev_flow_v_, flow_v, H, dev_container_size_.pitch);
        }
        last_run_ok_ = ok;
    }
    Release(dev_frame_0_);
    Release(dev_frame_1_);
    Release(dev_flow_u_);
    Release(dev_flow_v_);
}

namespace {
// Everything a recorded pyramid depends on: which entry recorded it ('P': a pair or a tall group through
// ComputeFlowDevice, 'G': a group gathered from scattered planes -- a group of ONE scattered pair names the same four
// planes as the pair entry but records gather -> pyramid of one instance -> hand back), the number of instances, the
// caller buffers and the nine (+1) parameters.
std::vector<unsigned char> GraphKey(char entry, size_t instances, const std::vector<DevicePtr>& planes, OperationParameters& params)
{
    std::vector<unsigned char> key;
    auto put = [&key](const void* p, size_t n) {
        const unsigned char* q = static_cast<const unsigned char*>(p);
        key.insert(key.end(), q, q + n);
    };
    put(&entry, sizeof(entry));
    put(&instances, sizeof(instances));
    put(planes.data(), planes.size() * sizeof(DevicePtr));
    const char* size_keys[] = {"warp_levels_count", "outer_iterations_count", "inner_iterations_count", "median_radius"};
    const char* float_keys[] = {"warp_scale_factor", "equation_alpha", "equation_smoothness", "equation_data",
                                "gaussian_sigma"};
    for (const char* k : size_keys) {
        size_t v = ~size_t(0);
        params.Read<size_t>(k, v);
        put(&v, sizeof(v));
    }
    for (const char* k : float_keys) {
        float v = -1.f;
        params.Read<float>(k, v);
        put(&v, sizeof(v));
    }
    int algorithm = FLOW2D_SOLVER_AUTO;
    params.Read<int>("solver_algorithm", algorithm);
    put(&algorithm, sizeof(algorithm));
    float sor_omega = 0.f;
    params.Read<float>("solver_sor_omega", sor_omega);
    put(&sor_omega, sizeof(sor_omega));
    return key;
}
}  // namespace

void OpticalFlow2D::DropGraphs()
{
    for (auto& kv : graphs_)
        if (kv.second.exec && context_) flow2d_graph_destroy(context_, kv.second.exec);
    graphs_.clear();
}

// Replays the graph recorded under `key`, recording it first (by running `queue` under stream capture) when the
// combination is new.
bool OpticalFlow2D::ReplayOrRecord(std::vector<unsigned char> key, const std::function<bool()>& queue)
{
    auto it = graphs_.find(key);
    if (it == graphs_.end()) {
        if (graphs_.size() >= kMaxGraphs) {
            // full: the least recently replayed graph goes.  It may still be running on the stream (replays are not
            // synchronised by contract), so the stream is drained first.
            flow2d_synchronize(context_);
            auto oldest = graphs_.begin();
            for (auto g = graphs_.begin(); g != graphs_.end(); ++g)
                if (g->second.last_use < oldest->second.last_use) oldest = g;
            if (oldest->second.exec) flow2d_graph_destroy(context_, oldest->second.exec);
            graphs_.erase(oldest);
        }
        if (CheckFlow2DError(flow2d_capture_begin(context_), "flow2d_capture_begin")) return false;
        const bool queued = queue();
        void* exec = nullptr;
        const bool ended = !CheckFlow2DError(flow2d_capture_end(context_, &exec), "flow2d_capture_end");
        if (!queued || !ended) {
            if (exec) flow2d_graph_destroy(context_, exec);
            return false;
        }
        it = graphs_.emplace(std::move(key), RecordedGraph{exec, 0}).first;
    }
    it->second.last_use = ++graph_clock_;
    return !CheckFlow2DError(flow2d_graph_launch(context_, it->second.exec), "flow2d_graph_launch");
}

bool OpticalFlow2D::ComputeFlowDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_flow_u,
                                      DevicePtr dev_flow_v, OperationParameters& params)
{
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || !dev_flow_u || !dev_flow_v) return false;
    active_group_ = group_;
    if (!use_graph || timing_mode != 0) return QueuePair(dev_frame_0, dev_frame_1, dev_flow_u, dev_flow_v, params);
    return ReplayOrRecord(GraphKey('P', group_, {dev_frame_0, dev_frame_1, dev_flow_u, dev_flow_v}, params), [&] {
        return QueuePair(dev_frame_0, dev_frame_1, dev_flow_u, dev_flow_v, params);
    });
}

bool OpticalFlow2D::ComputeFlowGroupDevice(size_t count, const DevicePtr* dev_frames_0, const DevicePtr* dev_frames_1,
                                           const DevicePtr* dev_flows_u, const DevicePtr* dev_flows_v,
                                           OperationParameters& params)
{
    if (!IsInitialized() || !dev_frames_0 || !dev_frames_1 || !dev_flows_u || !dev_flows_v) return false;
    if (count == 0 || count > group_) {
        std::printf("Error: '%s': a group of %zu pairs (1..%zu).\n", GetName(), count, group_);
        return false;
    }
    std::vector<DevicePtr> planes;
    for (size_t g = 0; g < count; ++g) {
        if (!dev_frames_0[g] || !dev_frames_1[g] || !dev_flows_u[g] || !dev_flows_v[g]) return false;
        planes.insert(planes.end(), {dev_frames_0[g], dev_frames_1[g], dev_flows_u[g], dev_flows_v[g]});
    }
    // Pairs whose planes already sit one container apart -- frame 0 of pair g exactly GroupStrideBytes() * g behind frame 0 of pair 0,
    // and so for frame 1, u and v: a caller that keeps a group's pairs in four tall allocations -- ARE a group as laid out: the
    // pyramid runs on the caller's planes, nothing is gathered or handed back (round 6: the two copies were 4.4 % of a 4096^2 group
    // of eight, 5.8 % of a 1024^2 group of 32).
    const size_t stride = GroupStrideBytes();
    bool in_place = true;
    for (size_t g = 1; g < count && in_place; ++g)
        in_place = dev_frames_0[g] == dev_frames_0[0] + g * stride && dev_frames_1[g] == dev_frames_1[0] + g * stride &&
                   dev_flows_u[g] == dev_flows_u[0] + g * stride && dev_flows_v[g] == dev_flows_v[0] + g * stride;
    if (in_place) {
        auto queue = [&] {
            active_group_ = count;
            const bool ok = QueuePair(dev_frames_0[0], dev_frames_1[0], dev_flows_u[0], dev_flows_v[0], params);
            active_group_ = group_;
            return ok;
        };
        if (!use_graph || timing_mode != 0) return queue();
        return ReplayOrRecord(GraphKey('I', count, {dev_frames_0[0], dev_frames_1[0], dev_flows_u[0], dev_flows_v[0]}, params), queue);
    }
    for (DevicePtr& p : group_staging_) {  // the tall staging containers, at the first scattered group
        if (p) continue;
        void* plane = nullptr;
        size_t pitch = 0;
        if (CheckFlow2DError(flow2d_plane_alloc(context_, dev_container_size_.width, dev_container_size_.height * group_,
                                                &plane, &pitch),
                             "flow2d_plane_alloc") ||
            pitch != dev_container_size_.pitch)
            return false;
        p = static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane));
    }
    if (!use_graph || timing_mode != 0)
        return QueueScatteredGroup(count, dev_frames_0, dev_frames_1, dev_flows_u, dev_flows_v, params);
    return ReplayOrRecord(GraphKey('G', count, planes, params), [&] {
        return QueueScatteredGroup(count, dev_frames_0, dev_frames_1, dev_flows_u, dev_flows_v, params);
    });
}

// gather the frames -> the group's pyramid on the staging containers -> hand the flows back
bool OpticalFlow2D::QueueScatteredGroup(size_t count, const DevicePtr* dev_frames_0, const DevicePtr* dev_frames_1,
                                        const DevicePtr* dev_flows_u, const DevicePtr* dev_flows_v,
                                        OperationParameters& params)
{
    const size_t stride = GroupStrideBytes();
    auto slot = [&](int which, size_t g) -> void* { return reinterpret_cast<char*>(AsPlane(group_staging_[which])) + g * stride; };
    std::vector<const void*> src;
    std::vector<void*> dst;
    for (size_t g = 0; g < count; ++g) {
        src.push_back(AsPlane(dev_frames_0[g])), dst.push_back(slot(0, g));
        src.push_back(AsPlane(dev_frames_1[g])), dst.push_back(slot(1, g));
    }
    // one launch per FLOW2D_COPY_PLANES_MAX planes (the pointer tables travel in the kernel arguments): groups of up to 32
    // pairs gather with one launch, the largest (64) with two
    auto copy_planes = [&]() {
        for (size_t first = 0; first < src.size(); first += FLOW2D_COPY_PLANES_MAX) {
            const size_t n = std::min<size_t>(FLOW2D_COPY_PLANES_MAX, src.size() - first);
            if (CheckFlow2DError(flow2d_copy_planes(context_, n, src.data() + first, dst.data() + first, dev_container_size_.pitch,
                                                    dev_container_size_.width, dev_container_size_.height),
                                 "flow2d_copy_planes"))
                return false;
        }
        return true;
    };
    if (!copy_planes()) return false;
    active_group_ = count;
    const bool ok = QueuePair(group_staging_[0], group_staging_[1], group_staging_[2], group_staging_[3], params);
    active_group_ = group_;
    if (!ok) return false;
    src.clear(), dst.clear();
    for (size_t g = 0; g < count; ++g) {
        src.push_back(slot(2, g)), dst.push_back(AsPlane(dev_flows_u[g]));
        src.push_back(slot(3, g)), dst.push_back(AsPlane(dev_flows_v[g]));
    }
    return copy_planes();
}

bool OpticalFlow2D::QueuePair(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_flow_u,
                              DevicePtr dev_flow_v, OperationParameters& params)
{
    const size_t bytes = dev_container_size_.pitch * dev_container_size_.height;
    // a lock-step group: from here to the end of the run every launch, memset and device copy of this context acts on
    // all group_ pairs (instance g of every plane, pool and caller alike, GroupStrideBytes() * g behind its pointer)
    if (group_ > 1 && CheckFlow2DError(flow2d_context_set_batch(context_, active_group_, GroupStrideBytes()), "flow2d_context_set_batch"))
        return false;
    dev_frame_0_ = Acquire();
    dev_frame_1_ = Acquire();
    dev_flow_u_ = Acquire();
    dev_flow_v_ = Acquire();
    // The pyramid consumes its frame planes (level-0 swaps), so without a pre-blur it works on copies; with one
    // the blur is the only reader of the frames and reads the caller's planes in place.  The flow of the last
    // level leaves through its median, which writes the caller's planes directly.
    float gaussian_sigma = 0.f;
    params.Read<float>("gaussian_sigma", gaussian_sigma);
    const bool frames_in_place = gaussian_sigma > 0.f;
    bool ok = true;
    if (frames_in_place) {
        caller_frame_0_ = dev_frame_0;
        caller_frame_1_ = dev_frame_1;
    } else {
        ok = !CheckFlow2DError(flow2d_copy_d2d(context_, AsPlane(dev_frame_0_), AsPlane(dev_frame_0), bytes), "copy") &&
             !CheckFlow2DError(flow2d_copy_d2d(context_, AsPlane(dev_frame_1_), AsPlane(dev_frame_1), bytes), "copy");
    }
    caller_flow_u_ = dev_flow_u;
    caller_flow_v_ = dev_flow_v;
    ok = ok && RunPyramid(params);
    caller_frame_0_ = caller_frame_1_ = caller_flow_u_ = caller_flow_v_ = 0;
    Release(dev_frame_0_);
    Release(dev_frame_1_);
    Release(dev_flow_u_);
    Release(dev_flow_v_);
    if (group_ > 1) flow2d_context_set_batch(context_, 1, 0);
    return ok;
}

// The coarse-to-fine loop on device planes: pre-blur, then per level { resample frames from full
// resolution, resample the flow from the previous level, warp frame 1, solve, u += du, median }.
// Order, buffer roles and float level-size arithmetic follow optical_flow_2d.cpp:160-449.
// On entry dev_frame_0_/1_ hold the frames; on success dev_flow_u_/v_ hold the flow.
bool OpticalFlow2D::RunPyramid(OperationParameters& params)
{
    size_t warp_levels_count = 0, outer_iterations_count = 0, inner_iterations_count = 0, median_radius = 0;
    float warp_scale_factor = 0.f, equation_alpha = 0.f, equation_smoothness = 0.f, equation_data = 0.f;
    float gaussian_sigma = 0.f;
    struct {
        const char* key;
        bool ok;
    } reads[] = {
        {"warp_levels_count", params.Read<size_t>("warp_levels_count", warp_levels_count)},
        {"warp_scale_factor", params.Read<float>("warp_scale_factor", warp_scale_factor)},
        {"outer_iterations_count", params.Read<size_t>("outer_iterations_count", outer_iterations_count)},
        {"inner_iterations_count", params.Read<size_t>("inner_iterations_count", inner_iterations_count)},
        {"equation_alpha", params.Read<float>("equation_alpha", equation_alpha)},
        {"equation_smoothness", params.Read<float>("equation_smoothness", equation_smoothness)},
        {"equation_data", params.Read<float>("equation_data", equation_data)},
        {"median_radius", params.Read<size_t>("median_radius", median_radius)},
        {"gaussian_sigma", params.Read<float>("gaussian_sigma", gaussian_sigma)},
    };
    for (const auto& r : reads)
        if (!r.ok) {
            std::printf("Operation: '%s'. Missing parameter '%s'.\n", GetName(), r.key);
            return false;
        }
    int solver_algorithm = FLOW2D_SOLVER_AUTO;
    params.Read<int>("solver_algorithm", solver_algorithm);
    float solver_sor_omega = 0.f;
    params.Read<float>("solver_sor_omega", solver_sor_omega);

    DataSize3 original_size = {dev_container_size_.width, dev_container_size_.height, 0};
    const size_t max_level = GetMaxWarpLevel(original_size.width, original_size.height, warp_scale_factor);
    int level = static_cast<int>(std::min(warp_levels_count, max_level)) - 1;
    if (level < 0 || !(warp_scale_factor < 1.f)) {
        // the reference would skip the loop and hand back stale buffers: refuse instead
        std::printf("Error: '%s': no pyramid level to run (levels %zu, scale %g).\n", GetName(), warp_levels_count,
                    warp_scale_factor);
        return false;
    }

    {  // widths the median operator accepts: 1 (copy), 3..8 (even widths use width - 1); anything else would
       // make the reference swap in a stale buffer (cuda_operation_median_2d.cpp:150-152)
        const size_t eff = (median_radius != 1 && median_radius % 2 == 0) ? median_radius - 1 : median_radius;
        if (!(median_radius == 1 || (median_radius != 2 && eff >= 3 && eff <= 7))) {
            std::printf("Error. Wrong median raduis (%zu). Supported values: 3, 5, 7\n", median_radius);
            return false;
        }
    }

    flow2d_timing_enable(context_, timing_mode);
    // per-launch brackets (mode 2) only on the finest level: that is the kernel the roofline is quoted on
    flow2d_timing_launch_filter(context_, dev_container_size_.width, dev_container_size_.height);

    DevicePtr frame_0 = dev_frame_0_, frame_1 = dev_frame_1_, flow_u = dev_flow_u_, flow_v = dev_flow_v_;
    DevicePtr frame_0_res = Acquire(), frame_1_res = Acquire(), flow_du = Acquire(), flow_dv = Acquire();
    OperationParameters op;
    // The operators' Execute() is void, like the reference's, whose ComputeFlow never learns of a failed launch and
    // swaps the stale output plane in.  Here every operator's failure flag is collected and the
    // run is abandoned at the end of the level it happened in: ComputeFlow then leaves the caller's flow untouched,
    // ComputeFlowDevice returns false and no graph of the broken run is kept.
    bool failed = false;

    const bool sequence = sequence_frames_[0] != nullptr;

    // The reference resamples both frames from FULL resolution at every level (optical_flow_2d.cpp:284-303): one read
    // of each frame per level.  Here the x passes of all levels > 0 are one trip over the frames (every row read once,
    // the x-resampled rows of all levels written side by side into a packed plane per frame; same cell sums, same
    // bits); a level's y pass then reads its segment.  Used when the segments fit one row (scale factors up to ~0.5).
    std::vector<size_t> packed_width, packed_column;
    bool packed = false;
    if (!sequence && level >= 2 && original_size.width <= 15360 && level <= FLOW2D_RESAMPLE_MAX_LEVELS) {
        size_t column = 0;
        for (int l = level; l >= 1; --l) {
            const float s = std::pow(warp_scale_factor, static_cast<float>(l));
            const size_t lw = static_cast<size_t>(std::ceil(original_size.width * s));
            packed_width.push_back(lw);
            packed_column.push_back(column);
            column += (lw + 3) / 4 * 4;  // 16-byte aligned segments (what a plane pointer must be)
        }
        packed = column <= dev_container_size_.pitch / sizeof(float);
    }
    const int first_level = level;
    // Round 6: with the x passes done in one trip, the y passes of ALL levels are one launch too (flow2d_resample_y_levels; they were
    // seven launches of 7-39 us for a config-3 pair, most of them far too small to fill the device).  Every level then needs a plane
    // region of its own: the levels sit one below the other in the two planes that otherwise hold "the current level's frames"
    // (their heights sum to less than the container's for scale factors up to 0.5), and the warp of a level writes the plane kept
    // for it instead of replacing the level's frame 1.  Same kernels' arithmetic on the same values: same bits.
    std::vector<size_t> level_row(static_cast<size_t>(first_level) + 1, 0), level_width(level_row.size(), 0), level_height(level_row.size(), 0);
    bool stacked = false;
    if (packed && level_warp_plane_) {
        size_t rows = 0;
        for (int l = first_level; l >= 1; --l) {
            const float s = std::pow(warp_scale_factor, static_cast<float>(l));
            level_row[static_cast<size_t>(l)] = rows;
            level_width[static_cast<size_t>(l)] = static_cast<size_t>(std::ceil(original_size.width * s));
            level_height[static_cast<size_t>(l)] = static_cast<size_t>(std::ceil(original_size.height * s));
            rows += level_height[static_cast<size_t>(l)];
        }
        stacked = rows <= dev_container_size_.height;
    }

    if (sequence) {  // a frame's level 0 is blurred once (or is the caller's own plane) and then only read
        DevicePtr callers[2] = {caller_frame_0_, caller_frame_1_};
        DevicePtr* level0[2] = {&frame_0, &frame_1};
        DevicePtr temp = Acquire();
        for (int i = 0; i < 2; ++i) {
            FramePyramid& pyramid = *sequence_frames_[i];
            if (gaussian_sigma > 0.0) {
                pyramid.level0 = pyramid.blurred;
                if (!pyramid.valid) {
                    op.Clear();
                    op.PushValuePtr("dev_input", &callers[i]);
                    op.PushValuePtr("dev_output", &pyramid.level0);
                    op.PushValuePtr("dev_temp", &temp);
                    op.PushValuePtr("data_size", &original_size);
                    op.PushValuePtr("gaussian_sigma", &gaussian_sigma);
                    cuop_convolution_.Execute(op);
                failed |= cuop_convolution_.TakeFailure();
                }
            } else {
                pyramid.level0 = callers[i];
            }
            *level0[i] = pyramid.level0;
        }
        Release(temp);
    } else if (gaussian_sigma > 0.0 && caller_frame_0_) {  // frames still in the caller's planes: blur them into ours
        DevicePtr temp = Acquire();
        DevicePtr sources[2] = {caller_frame_0_, caller_frame_1_};
        DevicePtr* targets[2] = {&frame_0, &frame_1};
        for (int i = 0; i < 2; ++i) {
            op.Clear();
            op.PushValuePtr("dev_input", &sources[i]);
            op.PushValuePtr("dev_output", targets[i]);
            op.PushValuePtr("dev_temp", &temp);  // (not touched: the blur is one launch)
            op.PushValuePtr("data_size", &original_size);
            op.PushValuePtr("gaussian_sigma", &gaussian_sigma);
            cuop_convolution_.Execute(op);
            failed |= cuop_convolution_.TakeFailure();
        }
        Release(temp);
    } else if (gaussian_sigma > 0.0) {  // optical_flow_2d.cpp:218-246: blur into the flow planes, then swap roles
        DevicePtr temp = Acquire();
        DevicePtr* io[2][2] = {{&frame_0, &flow_u}, {&frame_1, &flow_v}};
        for (auto& pair : io) {
            op.Clear();
            op.PushValuePtr("dev_input", pair[0]);
            op.PushValuePtr("dev_output", pair[1]);
            op.PushValuePtr("dev_temp", &temp);
            op.PushValuePtr("data_size", &original_size);
            op.PushValuePtr("gaussian_sigma", &gaussian_sigma);
            cuop_convolution_.Execute(op);
            failed |= cuop_convolution_.TakeFailure();
            std::swap(*pair[0], *pair[1]);
        }
        Release(temp);
    }

    if (packed) {
        if (CheckFlow2DError(flow2d_resample_x_levels(context_, AsPlane(frame_0), AsPlane(packed_frames_[0]),
                                                      AsPlane(frame_1), AsPlane(packed_frames_[1]),
                                                      original_size.width, original_size.height,
                                                      dev_container_size_.pitch, packed_width.size(),
                                                      packed_width.data(), packed_column.data()),
                             "flow2d_resample_x_levels"))
            failed = true;
        if (stacked) {  // every level's y pass, both frames, one launch
            std::vector<size_t> widths, heights, rows;
            for (int l = first_level; l >= 1; --l) {
                widths.push_back(level_width[static_cast<size_t>(l)]);
                heights.push_back(level_height[static_cast<size_t>(l)]);
                rows.push_back(level_row[static_cast<size_t>(l)]);
            }
            if (CheckFlow2DError(flow2d_resample_y_levels(context_, AsPlane(packed_frames_[0]), AsPlane(frame_0_res), AsPlane(packed_frames_[1]),
                                                          AsPlane(frame_1_res), original_size.height, dev_container_size_.pitch, widths.size(),
                                                          widths.data(), heights.data(), packed_column.data(), rows.data()),
                                 "flow2d_resample_y_levels"))
                failed = true;
        }
    }

    DataSize3 current_size = {0, 0, 0}, prev_size = {0, 0, 0};
    for (; level >= 0; --level) {
        const float scale = std::pow(warp_scale_factor, static_cast<float>(level));
        current_size.width = static_cast<size_t>(std::ceil(original_size.width * scale));
        current_size.height = static_cast<size_t>(std::ceil(original_size.height * scale));
        float hx = original_size.width / static_cast<float>(current_size.width);
        float hy = original_size.height / static_cast<float>(current_size.height);
        if (!silent) std::printf("Solve level %2d (%4zu x%4zu) \n", level, current_size.width, current_size.height);

        // frames: level 0 uses the (blurred) full-resolution planes, others are resampled from them
        DevicePtr sequence_level[2] = {frame_0, frame_1};  // sequence only: this level's read-only frame planes
        if (sequence) {
            DevicePtr temp = level > 0 ? Acquire() : 0;
            for (int i = 0; i < 2 && level > 0; ++i) {
                FramePyramid& pyramid = *sequence_frames_[i];
                DevicePtr plane = SequenceLevelPlane(pyramid, static_cast<size_t>(level), current_size.height);
                if (!plane) {
                    Release(temp);
                    Release(frame_0_res);
                    Release(frame_1_res);
                    Release(flow_du);
                    Release(flow_dv);
                    return false;
                }
                if (!pyramid.valid) {
                    op.Clear();
                    op.PushValuePtr("dev_input", i == 0 ? &frame_0 : &frame_1);
                    op.PushValuePtr("dev_output", &plane);
                    op.PushValuePtr("dev_temp", &temp);
                    op.PushValuePtr("data_size", &original_size);
                    op.PushValuePtr("resample_size", &current_size);
                    cuop_resample_.Execute(op);
                failed |= cuop_resample_.TakeFailure();
                }
                sequence_level[i] = plane;
            }
            if (temp) Release(temp);
        } else if (stacked) {  // every level's frames are in place already
        } else if (level == 0) {
            std::swap(frame_0, frame_0_res);
            std::swap(frame_1, frame_1_res);
        } else if (packed) {  // x pass done for all levels: this level's y pass, both frames in one launch
            const size_t column = packed_column[static_cast<size_t>(first_level - level)];
            if (CheckFlow2DError(flow2d_resample_y_pair(context_, AsPlane(packed_frames_[0]) + column, AsPlane(frame_0_res),
                                                        AsPlane(packed_frames_[1]) + column, AsPlane(frame_1_res),
                                                        current_size.width, current_size.height, original_size.height,
                                                        dev_container_size_.pitch),
                                 "flow2d_resample_y_pair"))
                failed = true;
        } else {  // both frames of the level in one resample call (two planes per launch)
            DevicePtr temp = Acquire(), temp_b = Acquire();
            op.Clear();
            op.PushValuePtr("dev_input", &frame_0);
            op.PushValuePtr("dev_output", &frame_0_res);
            op.PushValuePtr("dev_temp", &temp);
            op.PushValuePtr("dev_input_b", &frame_1);
            op.PushValuePtr("dev_output_b", &frame_1_res);
            op.PushValuePtr("dev_temp_b", &temp_b);
            op.PushValuePtr("data_size", &original_size);
            op.PushValuePtr("resample_size", &current_size);
            cuop_resample_.Execute(op);
            failed |= cuop_resample_.TakeFailure();
            Release(temp_b);
            Release(temp);
        }

        // flow: zero at the coarsest level, otherwise previous level -> this level (no magnitude scaling).  Round 6: both ride with
        // the warp of the level (flow2d_upsample_registration_2d: the resample and the registration operators' arithmetic on the
        // same values in one launch -- (u, v) handed on in registers instead of through their planes; at the coarsest level the
        // zeros, over the level's region instead of two memsets of the whole container).
        const bool upsample = prev_size.width != 0;
        // backward registration of `level_1` by the level's flow into `output` (after bringing the flow to the level's size)
        auto warp = [&](DevicePtr level_0, DevicePtr level_1, DevicePtr output) {
            int err;
            if (upsample) {
                err = flow2d_upsample_registration_2d(context_, AsPlane(flow_u), AsPlane(flow_v), prev_size.width, prev_size.height,
                                                      AsPlane(flow_du), AsPlane(flow_dv), AsPlane(level_0), AsPlane(level_1),
                                                      current_size.width, current_size.height, dev_container_size_.pitch, hx, hy,
                                                      AsPlane(output));
                std::swap(flow_u, flow_du);
                std::swap(flow_v, flow_dv);
            } else {
                err = flow2d_upsample_registration_2d(context_, nullptr, nullptr, 0, 0, AsPlane(flow_u), AsPlane(flow_v), AsPlane(level_0),
                                                      AsPlane(level_1), current_size.width, current_size.height,
                                                      dev_container_size_.pitch, hx, hy, AsPlane(output));
            }
            if (CheckFlow2DError(err, "flow2d_upsample_registration_2d")) failed = true;
        };

        DevicePtr solve_frame_0 = frame_0_res;  // what the solver reads as frame 0 of this level
        DevicePtr solve_frame_1 = 0;            // ... and as (warped) frame 1: frame_1_res unless set
        if (stacked) {  // the level planes stay where the y pass of all levels put them; the warp writes the plane kept for it
            const size_t at = level > 0 ? level_row[static_cast<size_t>(level)] * dev_container_size_.pitch : 0;
            DevicePtr level_0 = (level > 0 ? frame_0_res : frame_0) + at, level_1 = (level > 0 ? frame_1_res : frame_1) + at;
            warp(level_0, level_1, level_warp_plane_);
            solve_frame_0 = level_0;
            solve_frame_1 = level_warp_plane_;
        } else if (sequence) {  // the level planes are kept for the next pair: warp into the pool plane, read the rest
            warp(sequence_level[0], sequence_level[1], frame_1_res);
            solve_frame_0 = sequence_level[0];
        } else {  // backward registration of frame 1 by the current flow; the warped frame replaces it
            DevicePtr temp = Acquire();
            warp(frame_0_res, frame_1_res, temp);
            std::swap(frame_1_res, temp);
            Release(temp);
        }

        {  // lagged-diffusivity fixed point: the hot loop
            DevicePtr phi = Acquire(), ksi = Acquire(), temp_du = Acquire(), temp_dv = Acquire();
            op.Clear();
            op.PushValuePtr("dev_frame_0", &solve_frame_0);
            op.PushValuePtr("dev_frame_1", solve_frame_1 ? &solve_frame_1 : &frame_1_res);
            op.PushValuePtr("dev_flow_u", &flow_u);
            op.PushValuePtr("dev_flow_v", &flow_v);
            op.PushValuePtr("dev_flow_du", &flow_du);
            op.PushValuePtr("dev_flow_dv", &flow_dv);
            op.PushValuePtr("dev_phi", &phi);
            op.PushValuePtr("dev_ksi", &ksi);
            op.PushValuePtr("dev_temp_du", &temp_du);
            op.PushValuePtr("dev_temp_dv", &temp_dv);
            op.PushValuePtr("data_constancy", &data_constancy_);
            op.PushValuePtr("outer_iterations_count", &outer_iterations_count);
            op.PushValuePtr("inner_iterations_count", &inner_iterations_count);
            op.PushValuePtr("equation_alpha", &equation_alpha);
            op.PushValuePtr("equation_smoothness", &equation_smoothness);
            op.PushValuePtr("equation_data", &equation_data);
            op.PushValuePtr("data_size", &current_size);
            op.PushValuePtr("hx", &hx);
            op.PushValuePtr("hy", &hy);
            op.PushValuePtr("solver_algorithm", &solver_algorithm);
            op.PushValuePtr("solver_sor_omega", &solver_sor_omega);
            cuop_solve_.silent = true;  // per-level printing would need a host wait; timings are collected instead
            cuop_solve_.Execute(op);
            failed |= cuop_solve_.TakeFailure();
            Release(phi);
            Release(ksi);
            Release(temp_du);
            Release(temp_dv);
        }

        prev_size = current_size;
        if (failed) break;

        {  // u += du, v += dv and the median of u and v after every level, the finest included -- one launch: the filter
           // reads u + du (a single rounded addition, add_2d.cu:33-46) as it goes, the plane of sums is never stored
            DevicePtr temp = Acquire(), temp_b = Acquire();
            // the last median of a ComputeFlowDevice run delivers the result into the caller's planes
            const bool deliver = level == 0 && caller_flow_u_ != 0 && caller_flow_v_ != 0;
            DevicePtr out_u = deliver ? caller_flow_u_ : temp, out_v = deliver ? caller_flow_v_ : temp_b;
            op.Clear();
            op.PushValuePtr("dev_input", &flow_u);
            op.PushValuePtr("dev_output", &out_u);
            op.PushValuePtr("dev_input_b", &flow_v);
            op.PushValuePtr("dev_output_b", &out_v);
            op.PushValuePtr("dev_addend", &flow_du);
            op.PushValuePtr("dev_addend_b", &flow_dv);
            op.PushValuePtr("data_size", &current_size);
            op.PushValuePtr("radius", &median_radius);
            cuop_median_.Execute(op);
            failed |= cuop_median_.TakeFailure();
            if (!deliver) {
                std::swap(flow_u, temp);
                std::swap(flow_v, temp_b);
            }
            Release(temp_b);
            Release(temp);
        }
    }

    // hand the roles back: the caller reads the flow from dev_flow_u_/v_ and releases all four
    if (!sequence) {  // (a sequence pair's frame planes belong to the sequence cache or to the caller)
        dev_frame_0_ = frame_0;
        dev_frame_1_ = frame_1;
    }
    dev_flow_u_ = flow_u;
    dev_flow_v_ = flow_v;
    Release(frame_0_res);
    Release(frame_1_res);
    Release(flow_du);
    Release(flow_dv);
    flow2d_timing_enable(context_, 0);
    if (failed) std::printf("Error: '%s': an operator failed; the flow of this run is not valid.\n", GetName());
    return !failed;
}
