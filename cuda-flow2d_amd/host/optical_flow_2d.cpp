#include "optical_flow_2d.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "host_entry.h"

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
        all_planes_.push_back(AsDevicePtr(plane));
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
        packed = AsDevicePtr(plane);
    }
    {  // ... and the plane the warp writes when the levels are stacked (RunPyramid); without it the levels are resampled one by one
        void* plane = nullptr;
        size_t got_pitch = 0;
        if (flow2d_plane_alloc(context_, dev_container_size_.width, dev_container_size_.height * group_, &plane, &got_pitch) == FLOW2D_OK) {
            if (got_pitch == pitch) level_warp_plane_[0] = AsDevicePtr(plane);
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
        for (OwnedPlanes* owned : owned_)  // everything beside the pool
            for (DevicePtr& p : *owned) {
                if (p) flow2d_plane_free(context_, AsPlane(p));
                p = 0;
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
    pyramid.levels[level] = AsDevicePtr(plane);
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
        pyramid.built = 0;
        if (gaussian_sigma > 0.f && !pyramid.blurred) {  // a plane for the blurred frame
            void* plane = nullptr;
            size_t pitch = 0;
            if (CheckFlow2DError(flow2d_plane_alloc(context_, dev_container_size_.width, dev_container_size_.height,
                                                    &plane, &pitch),
                                 "flow2d_plane_alloc") ||
                pitch != dev_container_size_.pitch)
                return false;
            pyramid.blurred = AsDevicePtr(plane);
        }
    }
    return true;
}

bool OpticalFlow2D::RunSequencePair(FramePyramid& first, FramePyramid& second, DevicePtr frame_0, DevicePtr frame_1,
                                    DevicePtr flow_u, DevicePtr flow_v, OperationParameters& params, DevicePtr prior_u, DevicePtr prior_v,
                                    size_t start_level)
{
    sequence_frames_[0] = &first;
    sequence_frames_[1] = &second;
    sequence_levels_run_ = 0;
    prior_u_ = prior_u;
    prior_v_ = prior_v;
    prior_start_level_ = start_level;
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
    prior_u_ = prior_v_ = 0;
    prior_start_level_ = 0;
    Release(dev_frame_0_);
    Release(dev_frame_1_);
    Release(dev_flow_u_);
    Release(dev_flow_v_);
    // the pair ran its levels from the top one down: with what was there before, the levels below that one are all built
    if (ok) {
        first.built = std::max(first.built, sequence_levels_run_);
        second.built = std::max(second.built, sequence_levels_run_);
    }
    return ok;
}

bool OpticalFlow2D::ComputeFlowSequenceDevice(const DevicePtr* dev_frames, size_t frame_count, const DevicePtr* dev_flows_u,
                                              const DevicePtr* dev_flows_v, OperationParameters& params)
{
    if (!IsInitialized() || !dev_frames || !dev_flows_u || !dev_flows_v || frame_count < 2) return false;
    if (RefuseGroup("sequences")) return false;
    for (size_t k = 0; k < frame_count; ++k)
        if (!dev_frames[k] || (k + 1 < frame_count && (!dev_flows_u[k] || !dev_flows_v[k]))) return false;
    if (!PrepareSequenceCache(params)) return false;
    bool ok = true;
    for (size_t k = 0; ok && k + 1 < frame_count; ++k) {
        FramePyramid& first = sequence_cache_[k % 2];          // frame k: built as the second frame of pair k-1
        FramePyramid& second = sequence_cache_[(k + 1) % 2];   // frame k+1: built by this pair
        second.built = 0;
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
    if (RefuseGroup("sequences")) return false;
    {  // a prior is the prior of ONE direction: there is none for the backward flow
        float reach = 0.f;
        int prior_level = 0;
        if (params.Read<float>("prior_reach", reach) || params.Read<int>("prior_level", prior_level)) {
            std::printf("Error: '%s': a prior flow and bidirectional flow do not combine (there is no prior for the backward flow).\n",
                        GetName());
            return false;
        }
    }
    // every plane written must be distinct from every other one and from the frames (which are only read)
    std::vector<DevicePtr> outputs;
    for (size_t k = 0; k + 1 < frame_count; ++k) {
        for (const DevicePtr* a : {dev_flows_u, dev_flows_v, dev_back_us, dev_back_vs, dev_occ_fwd, dev_occ_bwd})
            if (a) outputs.push_back(a[k]);
    }
    if (!WrittenPlanesOk(dev_frames, frame_count, outputs.data(), outputs.size(), "output plane")) return false;
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
        second.built = 0;
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
    if (RefuseGroup("sequences")) return;
    const size_t H = dev_container_size_.height;
    Data2D* images[8] = {&frame_0, &frame_1, &flow_u, &flow_v, &back_u, &back_v, &occlusion_0, &occlusion_1};
    if (!SizeCheck{dev_container_size_, GetName(), "frame / flow"}(images, 8)) return;
    if (!EnsurePlanes(bidirectional_planes_, 8)) return;
    HostCall call(context_, last_total_ms_);
    const DevicePtr* d = bidirectional_planes_.data();  // frame 0, frame 1, u, v, back u, back v, occlusion 0, occlusion 1
    bool ok = CopyData2DtoDevice(frame_0, d[0], H, dev_container_size_.pitch) &&
              CopyData2DtoDevice(frame_1, d[1], H, dev_container_size_.pitch);
    ok = ok && ComputeFlowBidirectionalDevice(d, 2, d + 2, d + 3, d + 4, d + 5, d + 6, d + 7, params);
    for (int i = 2; ok && i < 8; ++i) ok = CopyData2DFromDevice(d[i], *images[i], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

bool OpticalFlow2D::EnsurePlanes(DevicePtr* planes, size_t count)
{
    return AllocPlanes(context_, dev_container_size_, GetName(), planes, count);
}

bool OpticalFlow2D::DeviceScratch::Ensure(flow2d_context* context, size_t wanted)
{
    if (block[0] && bytes >= wanted) return true;
    if (block[0]) {
        flow2d_synchronize(context);  // queued work may still use the old one
        flow2d_plane_free(context, AsPlane(block[0]));
    }
    bytes = 0;
    block[0] = AllocDeviceBytes(context, wanted);
    if (block[0]) bytes = wanted;
    return block[0] != 0;
}

bool OpticalFlow2D::RefuseGroup(const char* what) const
{
    if (group_ > 1) std::printf("Error: '%s': %s and lock-step groups do not combine.\n", GetName(), what);
    return group_ > 1;
}

bool OpticalFlow2D::ReadRecord(void* host, const void* device, size_t bytes)
{
    return !CheckFlow2DError(flow2d_copy_d2h_2d(context_, host, bytes, device, bytes, bytes, 1), "flow2d_copy_d2h_2d");
}

bool OpticalFlow2D::HandBack(size_t count, const DevicePtr* src, const DevicePtr* dst)
{
    if (!dst[0]) return true;
    const void* from[2] = {AsPlane(src[0]), AsPlane(src[count - 1])};
    void* to[2] = {AsPlane(dst[0]), AsPlane(dst[count - 1])};
    return !CheckFlow2DError(flow2d_copy_planes(context_, count, from, to, dev_container_size_.pitch, dev_container_size_.width,
                                                dev_container_size_.height),
                             "flow2d_copy_planes");
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

bool OpticalFlow2D::PriorStartLevel(size_t width, size_t height, size_t warp_levels_count, float warp_scale_factor, float reach,
                                    int prior_level, size_t* start_level)
{
    if (!start_level) return false;
    if (!(std::isfinite(reach) && reach > 0.f) || prior_level < -1) {
        std::printf("Error: a prior flow takes a reach that is finite and > 0 (%g) and a start level >= 0 (%d).\n", reach, prior_level);
        return false;
    }
    OpticalFlow2D geometry;  // (GetMaxWarpLevel is pure host arithmetic)
    const size_t levels = std::min(warp_levels_count, geometry.GetMaxWarpLevel(width, height, warp_scale_factor));
    if (levels == 0 || !(warp_scale_factor < 1.f) || !(warp_scale_factor > 0.f)) {
        std::printf("Error: no pyramid level to run (levels %zu, scale %g).\n", warp_levels_count, warp_scale_factor);
        return false;
    }
    const size_t top = levels - 1;
    size_t level = 0;
    if (prior_level >= 0) {
        level = static_cast<size_t>(prior_level);
    } else {
        // a level whose pixels are `reach` full-resolution pixels or more: what the prior leaves to correct is a pixel there
        while (level < top && !(reach * std::pow(warp_scale_factor, static_cast<float>(level)) <= 1.f)) ++level;
    }
    *start_level = std::min(level, top);
    return true;
}

bool OpticalFlow2D::MeetsOwnPlane(DevicePtr plane) const
{
    const size_t bytes = GroupStrideBytes() * group_;
    auto meets = [&](DevicePtr own) { return own && plane < own + bytes && own < plane + bytes; };
    for (DevicePtr own : all_planes_)
        if (meets(own)) return true;
    return meets(packed_frames_[0]) || meets(packed_frames_[1]) || meets(level_warp_plane_[0]);
}

bool OpticalFlow2D::ComputeFlowFromPriorDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_prior_u, DevicePtr dev_prior_v,
                                               DevicePtr dev_flow_u, DevicePtr dev_flow_v, OperationParameters& params,
                                               PriorReport* report_out)
{
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || !dev_prior_u || !dev_prior_v || !dev_flow_u || !dev_flow_v) return false;
    if (RefuseGroup("a prior flow")) return false;
    size_t warp_levels_count = 0;
    float warp_scale_factor = 0.f, reach = 2.f;
    int prior_level = -1;
    if (!params.Read<size_t>("warp_levels_count", warp_levels_count) || !params.Read<float>("warp_scale_factor", warp_scale_factor)) {
        std::printf("Operation: '%s'. Missing parameter 'warp_levels_count' / 'warp_scale_factor'.\n", GetName());
        return false;
    }
    params.Read<float>("prior_reach", reach);
    if (params.Read<int>("prior_level", prior_level) && prior_level < 0) prior_level = -2;  // (a level that was given is >= 0)
    size_t start = 0;
    if (!PriorStartLevel(dev_container_size_.width, dev_container_size_.height, warp_levels_count, warp_scale_factor, reach, prior_level,
                         &start))
        return false;
    {  // the prior is read while the flow planes and the object's own planes are written
        const size_t bytes = GroupStrideBytes();
        const DevicePtr prior[2] = {dev_prior_u, dev_prior_v}, flow[2] = {dev_flow_u, dev_flow_v};
        for (DevicePtr p : prior) {
            bool meets = MeetsOwnPlane(p);
            for (DevicePtr f : flow) meets = meets || (p < f + bytes && f < p + bytes);
            if (meets) {
                std::printf("Error: '%s': a prior plane overlaps a flow plane or a plane of the object's own.\n", GetName());
                return false;
            }
        }
    }
    if (!prior_scratch_.Ensure(context_, sizeof(unsigned long long))) return false;
    active_group_ = group_;
    prior_u_ = dev_prior_u;
    prior_v_ = dev_prior_v;
    prior_start_level_ = start;
    bool ok;
    if (!use_graph || timing_mode != 0) {
        ok = QueuePair(dev_frame_0, dev_frame_1, dev_flow_u, dev_flow_v, params);
    } else {  // a recording holds the prior's addresses and the level it starts at
        std::vector<unsigned char> key = GraphKey('R', group_, {dev_frame_0, dev_frame_1, dev_flow_u, dev_flow_v, dev_prior_u, dev_prior_v}, params);
        const unsigned char* level_bytes = reinterpret_cast<const unsigned char*>(&start);
        key.insert(key.end(), level_bytes, level_bytes + sizeof(start));
        ok = ReplayOrRecord(std::move(key), [&] { return QueuePair(dev_frame_0, dev_frame_1, dev_flow_u, dev_flow_v, params); });
    }
    prior_u_ = prior_v_ = 0;
    prior_start_level_ = 0;
    if (ok && report_out) {
        report_out->start_level = start;
        report_out->levels_run = start + 1;
        ok = ReadRecord(&report_out->not_finite, prior_scratch_.At<>(), sizeof(report_out->not_finite));
        ok = !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
    }
    return ok;
}

void OpticalFlow2D::ComputeFlowFromPrior(Data2D& frame_0, Data2D& frame_1, Data2D& prior_u, Data2D& prior_v, Data2D& flow_u,
                                         Data2D& flow_v, OperationParameters& params, PriorReport* report_out)
{
    last_run_ok_ = false;
    if (!IsInitialized()) return;
    if (RefuseGroup("a prior flow")) return;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / prior / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In).Add(&prior_u, CallPlanes::In).Add(&prior_v, CallPlanes::In);
    planes.Add(&flow_u, CallPlanes::Out).Add(&flow_v, CallPlanes::Out);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    last_run_ok_ = planes.Upload() && ComputeFlowFromPriorDevice(d[0], d[1], d[2], d[3], d[4], d[5], params, report_out) && planes.Download();
}

bool OpticalFlow2D::ComputeFlowCorrelationSeededDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, float lo, float scale, int radius,
                                                       int range, int spacing, float min_score, DevicePtr dev_flow_u, DevicePtr dev_flow_v,
                                                       OperationParameters& params, DevicePtr dev_node_u, DevicePtr dev_node_v,
                                                       DevicePtr dev_node_score, flow2d_correlation_record* correlation_out,
                                                       PriorReport* report_out, DevicePtr dev_prior_u, DevicePtr dev_prior_v)
{
    if (!IsInitialized() || !dev_flow_u || !dev_flow_v || (dev_prior_u == 0) != (dev_prior_v == 0)) return false;
    if (RefuseGroup("a prior flow")) return false;
    if (!EnsurePlanes(prior_planes_, 2)) return false;
    const DevicePtr* prior = prior_planes_.data();
    PriorReport report;
    const bool ok = CorrelateDevice(dev_frame_0, dev_frame_1, lo, scale, radius, range, spacing, min_score, dev_node_u, dev_node_v,
                                    dev_node_score, correlation_out, prior[0], prior[1]) &&
                    ComputeFlowFromPriorDevice(dev_frame_0, dev_frame_1, prior[0], prior[1], dev_flow_u, dev_flow_v, params, &report);
    if (!ok) return false;
    if (report_out) *report_out = report;
    if (!dev_prior_u) return true;
    const DevicePtr copies[2] = {dev_prior_u, dev_prior_v};
    return HandBack(2, prior, copies) && !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize");
}

void OpticalFlow2D::ComputeFlowCorrelationSeeded(Data2D& frame_0, Data2D& frame_1, int radius, int range, int spacing, float min_score,
                                                 Data2D& flow_u, Data2D& flow_v, OperationParameters& params, Data2D* node_u,
                                                 Data2D* node_v, Data2D* node_score, flow2d_correlation_record* correlation_out,
                                                 PriorReport* report_out, Data2D* prior_u, Data2D* prior_v)
{
    last_run_ok_ = false;
    if (!IsInitialized() || (prior_u == nullptr) != (prior_v == nullptr)) return;
    if (RefuseGroup("a prior flow")) return;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In).Add(&flow_u, CallPlanes::Out).Add(&flow_v, CallPlanes::Out);
    planes.Add(prior_u, CallPlanes::Out).Add(prior_v, CallPlanes::Out);
    // the node planes: containers with no image of their size behind them, downloaded below
    planes.Add(nullptr, CallPlanes::Out, true).Add(nullptr, CallPlanes::Out, true).Add(nullptr, CallPlanes::Out, node_score != nullptr);
    if (!planes.SizesMatch()) return;
    float lo = 0.f, scale = 1.f;
    CorrelationRange(frame_0, frame_1, lo, scale);
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    if (!CorrelationArgsOk(W, H, lo, scale, radius, range, spacing, min_score)) return;
    size_t nw = 0, nh = 0;
    flow2d_correlation_grid(W, H, radius, spacing, &nw, &nh);
    Data2D* nodes[3] = {node_u, node_v, node_score};
    for (Data2D* image : nodes)
        if (image && (image->Width() != nw || image->Height() != nh)) {
            std::printf("Error: '%s': the node images are not %zu x %zu.\n", GetName(), nw, nh);
            return;
        }
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    bool ok = planes.Upload() &&
              ComputeFlowCorrelationSeededDevice(d[0], d[1], lo, scale, radius, range, spacing, min_score, d[2], d[3], params, d[6], d[7],
                                                 d[8], correlation_out, report_out, d[4], d[5]) &&
              planes.Download();
    for (int k = 0; ok && k < 3; ++k)
        if (nodes[k]) ok = CopyData2DFromDevice(d[6 + k], *nodes[k], H, dev_container_size_.pitch);
    last_run_ok_ = ok;
}

// ---- warm starts: the previous pair's flow as the prior --------------------------------------------------------------------------
bool OpticalFlow2D::WarmOptionsOk(const WarmOptions& options)
{
    const bool ok = options.fill_passes >= 0 && options.fill_passes <= FLOW2D_PROPAGATE_MAX_FILL && std::isfinite(options.photo_scale) &&
                    options.photo_scale >= 0.f && (options.tail < 0.f || options.tail < 1.f);  // (a NaN tail fails both)
    if (!ok)
        std::printf("Error: a warm start takes 0 .. %d fill passes (%d), a photometric scale that is finite and >= 0 (%g) and a tail < 0 "
                    "(no adaptation) or in [0, 1) (%g).\n",
                    FLOW2D_PROPAGATE_MAX_FILL, options.fill_passes, options.photo_scale, options.tail);
    return ok;
}

bool OpticalFlow2D::WarmNextReach(unsigned long long count, const unsigned long long* above, float tail, int reach_used, bool* redo,
                                  int* next_reach)
{
    if (!above || !redo || !next_reach || !(tail >= 0.f && tail < 1.f) || reach_used < 0 || reach_used > 3) return false;
    if (above[0] > count || above[1] > above[0] || above[2] > above[1]) return false;
    auto holds = [&](int t) { return count > 0 && static_cast<double>(above[t - 1]) / static_cast<double>(count) <= static_cast<double>(tail); };
    *redo = reach_used > 0 && !holds(reach_used);
    *next_reach = 0;
    for (int t = 3; t >= 1; --t)
        if (holds(t)) *next_reach = t;
    return true;
}

bool OpticalFlow2D::EnsureWarmScratch(WarmScratch& scratch)
{
    const size_t W = dev_container_size_.width, H = dev_container_size_.height;
    auto round_up = [](size_t bytes) { return (bytes + 15) / 16 * 16; };
    const size_t records = round_up(sizeof(flow2d_propagate_record)) + round_up(sizeof(flow2d_flow_error_stats));
    const size_t propagate_bytes = round_up(flow2d_propagate_flow_workspace_bytes(W, H, 1));
    const size_t error_bytes = round_up(flow2d_flow_error_workspace_bytes(W, H, 1));
    if (!warm_scratch_.Ensure(context_, records + propagate_bytes + error_bytes)) return false;
    scratch.record = warm_scratch_.At<flow2d_propagate_record>();
    scratch.stats = warm_scratch_.At<flow2d_flow_error_stats>(round_up(sizeof(flow2d_propagate_record)));
    scratch.propagate_workspace = warm_scratch_.At<>(records);
    scratch.error_workspace = warm_scratch_.At<>(records + propagate_bytes);
    scratch.error_workspace_bytes = error_bytes;
    return true;
}

bool OpticalFlow2D::QueuePropagation(DevicePtr flow_u, DevicePtr flow_v, DevicePtr mask, DevicePtr frame_from, DevicePtr frame_to, float step,
                                     const WarmOptions& options, DevicePtr out_u, DevicePtr out_v, const WarmScratch& scratch)
{
    return !CheckFlow2DError(flow2d_propagate_flow_2d(context_, AsPlane(flow_u), AsPlane(flow_v), mask ? AsPlane(mask) : nullptr,
                                                      frame_from ? AsPlane(frame_from) : nullptr, frame_to ? AsPlane(frame_to) : nullptr,
                                                      dev_container_size_.width, dev_container_size_.height, dev_container_size_.pitch, step,
                                                      options.photo_scale, options.fill_passes, AsPlane(out_u), AsPlane(out_v),
                                                      reinterpret_cast<unsigned long long*>(scratch.record), scratch.propagate_workspace),
                             "flow2d_propagate_flow_2d");
}

bool OpticalFlow2D::PropagateFlowDevice(DevicePtr dev_flow_u, DevicePtr dev_flow_v, DevicePtr dev_mask, DevicePtr dev_frame_from,
                                        DevicePtr dev_frame_to, float step, const WarmOptions& options, DevicePtr dev_out_u,
                                        DevicePtr dev_out_v, flow2d_propagate_record* record_out)
{
    if (!IsInitialized() || !dev_flow_u || !dev_flow_v || !dev_out_u || !dev_out_v) return false;
    if (RefuseGroup("a propagated flow")) return false;
    if (!WarmOptionsOk(options)) return false;
    if ((dev_frame_from == 0) != (dev_frame_to == 0)) {
        std::printf("Error: '%s': the photometric term takes both frames or neither.\n", GetName());
        return false;
    }
    WarmScratch scratch;
    if (!EnsureWarmScratch(scratch)) return false;
    bool ok = QueuePropagation(dev_flow_u, dev_flow_v, dev_mask, dev_frame_from, dev_frame_to, step, options, dev_out_u, dev_out_v, scratch);
    if (ok && record_out) {
        ok = ReadRecord(record_out, scratch.record, sizeof(*record_out));
        ok = !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize") && ok;
    }
    return ok;
}

bool OpticalFlow2D::ComputeFlowFromPreviousDevice(DevicePtr dev_frame_0, DevicePtr dev_frame_1, DevicePtr dev_prev_u, DevicePtr dev_prev_v,
                                                  DevicePtr dev_prev_mask, DevicePtr dev_prev_frame, DevicePtr dev_flow_u,
                                                  DevicePtr dev_flow_v, OperationParameters& params, const WarmOptions& options,
                                                  WarmReport* report_out)
{
    if (!IsInitialized() || !dev_frame_0 || !dev_frame_1 || !dev_prev_u || !dev_prev_v || !dev_flow_u || !dev_flow_v) return false;
    if (RefuseGroup("a warm start")) return false;
    if (!WarmOptionsOk(options)) return false;
    if (!EnsurePlanes(warm_planes_, 2)) return false;
    WarmScratch scratch;
    if (!EnsureWarmScratch(scratch)) return false;
    WarmReport report;
    report.mode = kWarmSeeded;
    bool ok = QueuePropagation(dev_prev_u, dev_prev_v, dev_prev_mask, dev_prev_frame, dev_prev_frame ? dev_frame_0 : 0, 1.f, options,
                               warm_planes_[0], warm_planes_[1], scratch);
    if (ok && report_out) ok = ReadRecord(&report.propagation, scratch.record, sizeof(report.propagation));
    ok = ok && ComputeFlowFromPriorDevice(dev_frame_0, dev_frame_1, warm_planes_[0], warm_planes_[1], dev_flow_u, dev_flow_v, params,
                                          report_out ? &report.prior : nullptr);  // (with a report it synchronises)
    if (ok && report_out) *report_out = report;
    return ok;
}

void OpticalFlow2D::ComputeFlowFromPrevious(Data2D& frame_0, Data2D& frame_1, Data2D& prev_u, Data2D& prev_v, Data2D* prev_mask,
                                            Data2D* prev_frame, Data2D& flow_u, Data2D& flow_v, OperationParameters& params,
                                            const WarmOptions& options, WarmReport* report_out)
{
    last_run_ok_ = false;
    if (!IsInitialized()) return;
    if (RefuseGroup("a warm start")) return;
    if (!WarmOptionsOk(options)) return;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / previous flow / flow");
    planes.Add(&frame_0, CallPlanes::In).Add(&frame_1, CallPlanes::In).Add(&prev_u, CallPlanes::In).Add(&prev_v, CallPlanes::In);
    planes.Add(&flow_u, CallPlanes::Out).Add(&flow_v, CallPlanes::Out);
    size_t next = 6, mask_at = 0, frame_at = 0;  // the optional inputs: a plane only where there is an image
    if (prev_mask) planes.Add(prev_mask, CallPlanes::In), mask_at = next++;
    if (prev_frame) planes.Add(prev_frame, CallPlanes::In), frame_at = next++;
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    last_run_ok_ = planes.Upload() &&
                   ComputeFlowFromPreviousDevice(d[0], d[1], d[2], d[3], mask_at ? d[mask_at] : 0, frame_at ? d[frame_at] : 0, d[4], d[5],
                                                 params, options, report_out) &&
                   planes.Download();
}

bool OpticalFlow2D::ComputeFlowSequenceWarmDevice(const DevicePtr* dev_frames, size_t frame_count, const DevicePtr* dev_flows_u,
                                                  const DevicePtr* dev_flows_v, OperationParameters& params, const WarmOptions& options,
                                                  WarmReport* reports)
{
    if (!IsInitialized() || !dev_frames || !dev_flows_u || !dev_flows_v || frame_count < 2) return false;
    if (RefuseGroup("sequences")) return false;
    if (!WarmOptionsOk(options)) return false;
    const size_t pairs = frame_count - 1;
    std::vector<DevicePtr> outputs(dev_flows_u, dev_flows_u + pairs);
    outputs.insert(outputs.end(), dev_flows_v, dev_flows_v + pairs);
    if (!WrittenPlanesOk(dev_frames, frame_count, outputs.data(), outputs.size(), "flow plane")) return false;
    const bool adaptive = options.tail >= 0.f;
    size_t warp_levels_count = 0;
    float warp_scale_factor = 0.f, prior_reach = 2.f;
    int prior_level = -1;
    if (!params.Read<size_t>("warp_levels_count", warp_levels_count) || !params.Read<float>("warp_scale_factor", warp_scale_factor)) {
        std::printf("Operation: '%s'. Missing parameter 'warp_levels_count' / 'warp_scale_factor'.\n", GetName());
        return false;
    }
    params.Read<float>("prior_reach", prior_reach);
    if (params.Read<int>("prior_level", prior_level) && prior_level < 0) prior_level = -2;  // (a level that was given is >= 0)
    int reach = 0;  // adaptive: the reach of the next seeded pair (0: it runs unseeded)
    if (adaptive) {
        if (prior_level != -1 || !(std::isfinite(prior_reach) && prior_reach > 0.f && prior_reach <= 3.f)) {
            std::printf("Error: '%s': an adaptive warm sequence takes a prior_reach in (0, 3] (%g) and no prior_level.\n", GetName(),
                        prior_reach);
            return false;
        }
        reach = static_cast<int>(std::ceil(prior_reach));
    }
    const size_t W = dev_container_size_.width, H = dev_container_size_.height, pitch = dev_container_size_.pitch;
    auto start_level = [&](float r, int level, size_t* start) { return PriorStartLevel(W, H, warp_levels_count, warp_scale_factor, r, level, start); };
    size_t fixed_start = 0;
    if (!adaptive && pairs > 1 && !start_level(prior_reach, prior_level, &fixed_start)) return false;
    if (!PrepareSequenceCache(params) || !EnsurePlanes(warm_planes_, 2) || !prior_scratch_.Ensure(context_, sizeof(unsigned long long)))
        return false;
    WarmScratch scratch;
    if (!EnsureWarmScratch(scratch)) return false;
    const DevicePtr prior[2] = {warm_planes_[0], warm_planes_[1]};
    // flow k against its prediction: the record of flow2d_flow_error_2d with the prediction as the ground truth (one host wait)
    auto score = [&](size_t k, flow2d_flow_error_stats& stats) {
        return !CheckFlow2DError(flow2d_flow_error_2d(context_, AsPlane(dev_flows_u[k]), AsPlane(dev_flows_v[k]), AsPlane(prior[0]),
                                                      AsPlane(prior[1]), nullptr, W, H, pitch, nullptr, nullptr, scratch.stats,
                                                      scratch.error_workspace, scratch.error_workspace_bytes),
                                 "flow2d_flow_error_2d") &&
               ReadRecord(&stats, scratch.stats, sizeof(stats)) && !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize");
    };
    bool ok = true;
    for (size_t k = 0; ok && k < pairs; ++k) {
        FramePyramid& first = sequence_cache_[k % 2];          // frame k: built, as far as pair k - 1 needed it, as its second frame
        FramePyramid& second = sequence_cache_[(k + 1) % 2];   // frame k + 1: built by this pair
        second.built = 0;
        WarmReport unasked;
        WarmReport& report = reports ? reports[k] : unasked;  // (the queued copies of the records land in the caller's entry itself)
        report = WarmReport();
        if (k == 0) {
            ok = RunSequencePair(first, second, dev_frames[0], dev_frames[1], dev_flows_u[0], dev_flows_v[0], params);
            continue;
        }
        // the prediction: flow k - 1 along itself onto frame k's grid, the frames k - 1 and k deciding between colliding vectors
        ok = QueuePropagation(dev_flows_u[k - 1], dev_flows_v[k - 1], 0, dev_frames[k - 1], dev_frames[k], 1.f, options, prior[0], prior[1],
                              scratch);
        if (ok && reports) ok = ReadRecord(&report.propagation, scratch.record, sizeof(report.propagation));
        if (!ok) break;
        size_t start = fixed_start;
        const bool seeded = !adaptive || reach > 0;
        if (adaptive && seeded && !start_level(static_cast<float>(reach), -1, &start)) return false;
        ok = seeded ? RunSequencePair(first, second, dev_frames[k], dev_frames[k + 1], dev_flows_u[k], dev_flows_v[k], params, prior[0],
                                      prior[1], start)
                    : RunSequencePair(first, second, dev_frames[k], dev_frames[k + 1], dev_flows_u[k], dev_flows_v[k], params);
        if (!ok) break;
        report.mode = seeded ? kWarmSeeded : kWarmUnseeded;
        if (seeded) {
            report.prior.start_level = start;
            report.prior.levels_run = start + 1;
            if (reports) ok = ReadRecord(&report.prior.not_finite, prior_scratch_.At<>(), sizeof(report.prior.not_finite));
        }
        if (adaptive) {
            report.reach = seeded ? reach : 0;
            flow2d_flow_error_stats stats;
            bool redo = false;
            ok = ok && score(k, stats) && WarmNextReach(stats.all.count, stats.all.above + 1, options.tail, report.reach, &redo, &reach);
            if (ok && redo) {  // the prior did not hold: the pair again, unseeded, into the same planes; then what that flow says
                report.mode = kWarmRedone;
                ok = RunSequencePair(first, second, dev_frames[k], dev_frames[k + 1], dev_flows_u[k], dev_flows_v[k], params) &&
                     score(k, stats) && WarmNextReach(stats.all.count, stats.all.above + 1, options.tail, 0, &redo, &reach);
            }
            for (int t = 0; ok && t < 3; ++t)
                report.share[t] = stats.all.count ? static_cast<double>(stats.all.above[t + 1]) / static_cast<double>(stats.all.count) : -1.0;
        }
    }
    // the reports are filled by copies queued on the stream: they are there once it has drained
    if (ok && reports && !adaptive) ok = !CheckFlow2DError(flow2d_synchronize(context_), "flow2d_synchronize");
    return ok;
}

void OpticalFlow2D::ComputeFlowSequenceWarm(Data2D* const* frames, size_t frame_count, Data2D* flows_u, Data2D* flows_v,
                                            OperationParameters& params, const WarmOptions& options, WarmReport* reports)
{
    last_run_ok_ = false;
    if (!IsInitialized() || !frames || !flows_u || !flows_v || frame_count < 2) return;
    if (RefuseGroup("sequences")) return;
    const size_t n = frame_count;
    CallPlanes planes(context_, dev_container_size_, GetName(), "frame / flow");
    planes.Add(frames, n, CallPlanes::In).Add(flows_u, n - 1, CallPlanes::Out).Add(flows_v, n - 1, CallPlanes::Out);
    if (!planes.SizesMatch()) return;
    HostCall call(context_, last_total_ms_, planes.Allocate());
    const DevicePtr* d = planes.data();
    last_run_ok_ = planes.Upload() && ComputeFlowSequenceWarmDevice(d, n, d + n, d + 2 * n - 1, params, options, reports) && planes.Download();
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
        p = AsDevicePtr(plane);
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
    // A run from a prior flow (ComputeFlowFromPriorDevice): the loop starts at the start level instead of at the top one, and that
    // level's warp takes the prior.  Everything decided from `level` below -- which frame pyramid path, the levels' plane regions --
    // is decided for the levels that run; every path gives a level's frames the same bits.
    const bool from_prior = prior_u_ != 0;
    if (from_prior) level = std::min(level, static_cast<int>(prior_start_level_));

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
    if (sequence) sequence_levels_run_ = static_cast<size_t>(level) + 1;

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
    if (packed && level_warp_plane_[0]) {
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
                if (pyramid.built == 0) {
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

    // The halving pyramid (every level a power-of-two fraction of the frame in both directions): the x and the y passes of all
    // levels in ONE launch that never writes the x-resampled rows (flow2d_resample_xy_levels; the same sums in the same order,
    // the same bits).  Whether it applies is the entry's own answer, given before any launch, to the geometry
    // (FLOW2D_ERR_UNSUPPORTED) and to where the planes lie (FLOW2D_ERR_INVALID_ARGUMENT: its alias check compares byte ranges,
    // the two launches below compare base pointers) -- neither changes between recording a graph and an eager run, so both take
    // the same path.  Everything else keeps the two launches, and the packed planes stay allocated for them (nothing else reads
    // them); a device error fails the run.
    std::vector<size_t> widths, heights, rows;  // the levels' regions in the stacked planes, from the finest to the coarsest
    if (stacked) {
        for (int l = first_level; l >= 1; --l) {
            widths.push_back(level_width[static_cast<size_t>(l)]);
            heights.push_back(level_height[static_cast<size_t>(l)]);
            rows.push_back(level_row[static_cast<size_t>(l)]);
        }
    }
    bool fused_levels = false;
    if (stacked) {
        const int status = flow2d_resample_xy_levels(context_, AsPlane(frame_0), AsPlane(frame_0_res), AsPlane(frame_1), AsPlane(frame_1_res),
                                                     original_size.width, original_size.height, dev_container_size_.pitch,
                                                     widths.size(), widths.data(), heights.data(), rows.data(), nullptr);
        fused_levels = status != FLOW2D_ERR_UNSUPPORTED && status != FLOW2D_ERR_INVALID_ARGUMENT;
        if (fused_levels && CheckFlow2DError(status, "flow2d_resample_xy_levels")) failed = true;
    }

    if (packed && !fused_levels) {
        if (CheckFlow2DError(flow2d_resample_x_levels(context_, AsPlane(frame_0), AsPlane(packed_frames_[0]),
                                                      AsPlane(frame_1), AsPlane(packed_frames_[1]),
                                                      original_size.width, original_size.height,
                                                      dev_container_size_.pitch, packed_width.size(),
                                                      packed_width.data(), packed_column.data()),
                             "flow2d_resample_x_levels"))
            failed = true;
        if (stacked &&  // every level's y pass, both frames, one launch
            CheckFlow2DError(flow2d_resample_y_levels(context_, AsPlane(packed_frames_[0]), AsPlane(frame_0_res), AsPlane(packed_frames_[1]),
                                                      AsPlane(frame_1_res), original_size.height, dev_container_size_.pitch, widths.size(),
                                                      widths.data(), heights.data(), packed_column.data(), rows.data()),
                             "flow2d_resample_y_levels"))
            failed = true;
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
                if (pyramid.built <= static_cast<size_t>(level)) {
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
        // A level exactly twice the previous one whose solver is the strips keeps its base flow (u, v) at the PREVIOUS level's size: at
        // such a level the up-sampled flow is a replication, so the warp stores one value per 2 x 2 block and the strips and the
        // median read [y >> 1][x >> 1] -- the same values, the same bits, a quarter of the bytes written once and read eleven times.
        // Decided here, from the geometry and the solver's own answer, before any launch: the same for an eager run and a recording.
        int base_flow_shift = 0;
        if (upsample && current_size.width == 2 * prev_size.width && current_size.height == 2 * prev_size.height) {
            flow2d_solve_params probe{};
            probe.width = current_size.width, probe.height = current_size.height;
            probe.pitch_bytes = dev_container_size_.pitch, probe.container_height = dev_container_size_.height;
            probe.hx = hx, probe.hy = hy;
            probe.equation_alpha = equation_alpha, probe.equation_smoothness = equation_smoothness, probe.equation_data = equation_data;
            probe.outer_iterations_count = outer_iterations_count, probe.inner_iterations_count = inner_iterations_count;
            probe.data_constancy = data_constancy_ == DataConstancy::Gradient          ? FLOW2D_CONSTANCY_GRADIENT
                                   : data_constancy_ == DataConstancy::LogDerivatives  ? FLOW2D_CONSTANCY_LOG_DERIVATIVES
                                   : data_constancy_ == DataConstancy::GradientUntiled ? FLOW2D_CONSTANCY_GRADIENT_UNTILED
                                                                                       : FLOW2D_CONSTANCY_GREY;
            probe.algorithm = solver_algorithm, probe.sor_omega = solver_sor_omega;
            const size_t window = (median_radius != 1 && median_radius % 2 == 0) ? median_radius - 1 : median_radius;
            if (window >= 3 && window <= 7 && flow2d_solve_level_takes_half_base(context_, &probe)) base_flow_shift = 1;
        }
        // backward registration of `level_1` by the level's flow into `output` (after bringing the flow to the level's size)
        auto warp = [&](DevicePtr level_0, DevicePtr level_1, DevicePtr output) {
            int err;
            if (upsample) {
                err = (base_flow_shift ? flow2d_upsample_registration_half_2d : flow2d_upsample_registration_2d)(
                    context_, AsPlane(flow_u), AsPlane(flow_v), prev_size.width, prev_size.height, AsPlane(flow_du), AsPlane(flow_dv),
                    AsPlane(level_0), AsPlane(level_1), current_size.width, current_size.height, dev_container_size_.pitch, hx, hy,
                    AsPlane(output));
                std::swap(flow_u, flow_du);
                std::swap(flow_v, flow_dv);
            } else if (from_prior) {  // the first level of a run from a prior: the prior at this level's size instead of zero
                err = flow2d_prior_registration_2d(context_, AsPlane(prior_u_), AsPlane(prior_v_), original_size.width, original_size.height,
                                                   AsPlane(flow_u), AsPlane(flow_v), AsPlane(level_0), AsPlane(level_1), current_size.width,
                                                   current_size.height, dev_container_size_.pitch, hx, hy, AsPlane(output),
                                                   prior_scratch_.At<unsigned long long>());
            } else {
                err = flow2d_upsample_registration_2d(context_, nullptr, nullptr, 0, 0, AsPlane(flow_u), AsPlane(flow_v), AsPlane(level_0),
                                                      AsPlane(level_1), current_size.width, current_size.height,
                                                      dev_container_size_.pitch, hx, hy, AsPlane(output));
            }
            if (CheckFlow2DError(err, upsample ? (base_flow_shift ? "flow2d_upsample_registration_half_2d" : "flow2d_upsample_registration_2d")
                                               : (from_prior ? "flow2d_prior_registration_2d" : "flow2d_upsample_registration_2d")))
                failed = true;
        };

        DevicePtr solve_frame_0 = frame_0_res;  // what the solver reads as frame 0 of this level
        DevicePtr solve_frame_1 = 0;            // ... and as (warped) frame 1: frame_1_res unless set
        if (stacked) {  // the level planes stay where the y pass of all levels put them; the warp writes the plane kept for it
            const size_t at = level > 0 ? level_row[static_cast<size_t>(level)] * dev_container_size_.pitch : 0;
            DevicePtr level_0 = (level > 0 ? frame_0_res : frame_0) + at, level_1 = (level > 0 ? frame_1_res : frame_1) + at;
            warp(level_0, level_1, level_warp_plane_[0]);
            solve_frame_0 = level_0;
            solve_frame_1 = level_warp_plane_[0];
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
            if (base_flow_shift) op.PushValuePtr("base_flow_shift", &base_flow_shift);
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
            if (base_flow_shift) op.PushValuePtr("base_flow_shift", &base_flow_shift);
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
