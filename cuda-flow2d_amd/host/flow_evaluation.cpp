#include "flow_evaluation.h"

#include <cmath>
#include <cstdio>
#include <cstdint>

#include "device_utils.h"

namespace {

// A device allocation freed on every path out of EvaluateFlow.
struct DevicePlane {
    void* ptr = nullptr;
    size_t pitch = 0;
    ~DevicePlane()
    {
        if (ptr) flow2d_plane_free(CurrentDeviceContext(), ptr);
    }
    bool Allocate(size_t width_floats, size_t height)
    {
        return !CheckFlow2DError(flow2d_plane_alloc(CurrentDeviceContext(), width_floats, height, &ptr, &pitch),
                                 "flow2d_plane_alloc");
    }
    DevicePtr Dev() const { return static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(ptr)); }
};

bool SameSize(Data2D& a, Data2D& b) { return a.Width() == b.Width() && a.Height() == b.Height(); }

std::string Number(double x)
{
    if (std::isnan(x)) return "NaN";
    if (std::isinf(x)) return x > 0 ? "Infinity" : "-Infinity";
    char buf[40];
    std::snprintf(buf, sizeof(buf), "%.17g", x);
    return buf;
}

std::string ClassJson(const flow2d_flow_error_class& c)
{
    const bool empty = c.count == 0;
    const double n = static_cast<double>(c.count);
    auto mean = [&](double s) { return empty ? std::string("null") : Number(s / n); };
    auto rate = [&](unsigned long long k) { return empty ? std::string("null") : Number(static_cast<double>(k) / n); };
    std::string s = "{\"count\": " + std::to_string(c.count);
    s += ", \"epe\": " + mean(c.sum_epe);
    s += ", \"rmse\": " + (empty ? std::string("null") : Number(std::sqrt(c.sum_epe_sq / n)));
    s += ", \"ae\": " + mean(c.sum_ae);
    s += ", \"r0.5\": " + rate(c.above[0]);
    s += ", \"r1\": " + rate(c.above[1]);
    s += ", \"r2\": " + rate(c.above[2]);
    s += ", \"r3\": " + rate(c.above[3]);
    s += ", \"fl\": " + rate(c.fl);
    s += ", \"max_epe\": " + Number(c.max_epe) + "}";
    return s;
}

}  // namespace

bool EvaluateFlow(Data2D& u, Data2D& v, Data2D& gt_u, Data2D& gt_v, Data2D* occlusion, flow2d_flow_error_stats& out,
                  Data2D* epe, Data2D* ae)
{
    flow2d_context* ctx = CurrentDeviceContext();
    const size_t w = u.Width(), h = u.Height();
    if (!ctx || w == 0 || h == 0 || !SameSize(u, v) || !SameSize(u, gt_u) || !SameSize(u, gt_v) ||
        (occlusion && !SameSize(u, *occlusion))) {
        std::printf("EvaluateFlow: %s\n", ctx ? "the estimate, the ground truth and the mask differ in size" : "no device context");
        return false;
    }
    Data2D* inputs[5] = {&u, &v, &gt_u, &gt_v, occlusion};
    DevicePlane planes[5], out_epe, out_ae, stats, workspace;
    for (int i = 0; i < 5; ++i) {
        if (!inputs[i]) continue;
        if (!planes[i].Allocate(w, h) || !CopyData2DtoDevice(*inputs[i], planes[i].Dev(), h, planes[i].pitch)) return false;
    }
    const size_t pitch = planes[0].pitch;
    const size_t ws_bytes = flow2d_flow_error_workspace_bytes(w, h, 1);
    if ((epe && !out_epe.Allocate(w, h)) || (ae && !out_ae.Allocate(w, h)) ||
        !stats.Allocate(sizeof(flow2d_flow_error_stats) / sizeof(float), 1) || !workspace.Allocate(ws_bytes / sizeof(float), 1))
        return false;
    const float* in[5];
    for (int i = 0; i < 5; ++i) in[i] = static_cast<const float*>(planes[i].ptr);
    if (CheckFlow2DError(flow2d_flow_error_2d(ctx, in[0], in[1], in[2], in[3], in[4], w, h, pitch, static_cast<float*>(out_epe.ptr),
                                              static_cast<float*>(out_ae.ptr),
                                              static_cast<flow2d_flow_error_stats*>(stats.ptr), workspace.ptr, ws_bytes),
                         "flow2d_flow_error_2d"))
        return false;
    flow2d_flow_error_stats rec;
    if (CheckFlow2DError(flow2d_copy_d2h_2d(ctx, &rec, sizeof(rec), stats.ptr, stats.pitch, sizeof(rec), 1), "flow2d_copy_d2h_2d"))
        return false;
    Data2D* per_pixel[2] = {epe, ae};
    DevicePlane* sources[2] = {&out_epe, &out_ae};
    for (int i = 0; i < 2; ++i) {
        if (!per_pixel[i]) continue;
        if (!SameSize(*per_pixel[i], u)) *per_pixel[i] = Data2D(w, h);
        if (!CopyData2DFromDevice(sources[i]->Dev(), *per_pixel[i], h, sources[i]->pitch)) return false;
    }
    if (CheckFlow2DError(flow2d_synchronize(ctx), "flow2d_synchronize")) return false;
    out = rec;
    return true;
}

std::string FlowErrorJson(const flow2d_flow_error_stats& stats)
{
    return "{\"all\": " + ClassJson(stats.all) + ", \"noc\": " + ClassJson(stats.noc) + ", \"occ\": " + ClassJson(stats.occ) +
           ", \"invalid_ground_truth\": " + std::to_string(stats.invalid_ground_truth) +
           ", \"nonfinite_estimate\": " + std::to_string(stats.nonfinite_estimate) + "}";
}
