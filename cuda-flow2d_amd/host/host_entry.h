// What the entries of OpticalFlow2D share: optical_flow_2d.cpp (the flow) and optical_flow_applications_2d.cpp (what is built on
// it).  Private to the host library: not installed and not included by optical_flow_2d.h.
#pragma once

#include <cstdint>
#include <cstdio>
#include <vector>

#include "data2d.h"
#include "data_structs.h"
#include "device_utils.h"

// Whether an entry may write the planes `written` while it reads the planes `read`: no null plane on either side, no written plane
// that is also read, no written plane twice.  `what` names the written planes in the message.  Plain host code: needs no device.
inline bool WrittenPlanesOk(const DevicePtr* read, size_t read_count, const DevicePtr* written, size_t written_count, const char* what)
{
    for (size_t k = 0; k < read_count; ++k)
        if (!read[k]) return false;
    for (size_t i = 0; i < written_count; ++i) {
        if (!written[i]) return false;
        for (size_t k = 0; k < read_count; ++k)
            if (written[i] == read[k]) {
                std::printf("Error: one of the %ss is one of the frames.\n", what);
                return false;
            }
        for (size_t j = i + 1; j < written_count; ++j)
            if (written[i] == written[j]) {
                std::printf("Error: the %ss must be distinct.\n", what);
                return false;
            }
    }
    return true;
}

inline DevicePtr AsDevicePtr(void* plane) { return static_cast<DevicePtr>(reinterpret_cast<uintptr_t>(plane)); }

// `bytes` of device memory (a one-row plane, 16-byte aligned); 0 on failure
inline DevicePtr AllocDeviceBytes(flow2d_context* context, size_t bytes)
{
    void* plane = nullptr;
    size_t pitch = 0;
    if (CheckFlow2DError(flow2d_plane_alloc(context, (bytes + 3) / 4, 1, &plane, &pitch), "flow2d_plane_alloc")) return 0;
    return AsDevicePtr(plane);
}

// A plane of the container's size for every entry of `planes` that has none yet (0); false when an allocation fails or comes with
// another pitch than the containers'.
inline bool AllocPlanes(flow2d_context* context, const DataSize3& size, const char* name, DevicePtr* planes, size_t count)
{
    for (size_t i = 0; i < count; ++i) {
        if (planes[i]) continue;
        void* plane = nullptr;
        size_t pitch = 0;
        if (CheckFlow2DError(flow2d_plane_alloc(context, size.width, size.height, &plane, &pitch), "flow2d_plane_alloc")) return false;
        planes[i] = AsDevicePtr(plane);
        if (pitch != size.pitch) {
            std::printf("Error: '%s': plane pitch %zu differs from the container pitch %zu.\n", name, pitch, size.pitch);
            return false;
        }
    }
    return true;
}

// The frame of a host-image entry.  From its construction to its destruction: the start line, two events around the uploads,
// the device work and the downloads, the entry's one host wait (on the second event), the total printed and left in
// `total_ms`.  An entry that allocated planes for this call alone names them in `per_call`: the stream is then drained and
// they are freed (the array must outlive the scope).
struct PlaneList {
    const DevicePtr* planes;
    size_t count;
};

class HostCall {
public:
    HostCall(flow2d_context* context, float& total_ms, PlaneList per_call = {nullptr, 0})
        : context_(context), total_ms_(total_ms), per_call_(per_call)
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
        if (!per_call_.planes) return;
        flow2d_synchronize(context_);
        for (size_t i = 0; i < per_call_.count; ++i)
            if (per_call_.planes[i]) flow2d_plane_free(context_, AsPlane(per_call_.planes[i]));
    }
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;

private:
    flow2d_context* context_;
    float& total_ms_;
    PlaneList per_call_;
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
};

// The device planes of one host-image call, one per image in the order the images are added: inputs are uploaded, outputs downloaded,
// and all of them are freed by the call's HostCall.  The planes of consecutive Add()s are consecutive in data(), so a run of them
// is the array a ...Device entry takes.
class CallPlanes {
public:
    enum Use { In, Out };

    CallPlanes(flow2d_context* context, const DataSize3& size, const char* name, const char* what)
        : context_(context), size_(size), check_{size, name, what}
    {
    }
    // A null Out image is one the caller does not want: it gets no plane (0 in data()) unless `always`, which is for a plane the
    // device entry is handed either way.  A null In image is refused by SizesMatch().
    CallPlanes& Add(Data2D* image, Use use, bool always = false)
    {
        entries_.push_back({image, use, image || always ? size_t(0) : kNoPlane});
        planes_.push_back(0);
        return *this;
    }
    CallPlanes& Add(Data2D* const* images, size_t count, Use use)  // (a null array: `count` null images)
    {
        for (size_t i = 0; i < count; ++i) Add(images ? images[i] : nullptr, use);
        return *this;
    }
    CallPlanes& Add(Data2D* images, size_t count, Use use)  // an array of images
    {
        for (size_t i = 0; i < count; ++i) Add(images ? images + i : nullptr, use);
        return *this;
    }
    // `count` blocks of `bytes` with no image behind them (the caller moves what they hold)
    CallPlanes& AddBytes(size_t bytes, size_t count)
    {
        entries_.insert(entries_.end(), count, {nullptr, Out, bytes});
        planes_.insert(planes_.end(), count, 0);
        return *this;
    }

    bool SizesMatch() const
    {
        for (const Entry& e : entries_)
            if ((e.image || e.use == In) && !check_(&e.image, 1)) return false;
        return true;
    }
    // Allocates the planes and returns them for the call's HostCall, which frees them -- those of a failed allocation too:
    // Upload() then reports the failure.
    PlaneList Allocate()
    {
        allocated_ = true;
        for (size_t i = 0; allocated_ && i < entries_.size(); ++i) {
            if (entries_[i].bytes == kNoPlane) continue;
            if (entries_[i].bytes) allocated_ = (planes_[i] = AllocDeviceBytes(context_, entries_[i].bytes)) != 0;
            else allocated_ = AllocPlanes(context_, size_, check_.name, &planes_[i], 1);
        }
        return {planes_.data(), planes_.size()};
    }
    bool Upload()
    {
        bool ok = allocated_;
        for (size_t i = 0; ok && i < entries_.size(); ++i)
            if (entries_[i].use == In) ok = CopyData2DtoDevice(*entries_[i].image, planes_[i], size_.height, size_.pitch);
        return ok;
    }
    bool Download(size_t i) { return !entries_[i].image || CopyData2DFromDevice(planes_[i], *entries_[i].image, size_.height, size_.pitch); }
    bool Download()  // every Out image that was asked for, in the order of the Add()s
    {
        bool ok = true;
        for (size_t i = 0; ok && i < entries_.size(); ++i)
            if (entries_[i].use == Out) ok = Download(i);
        return ok;
    }
    const DevicePtr* data() const { return planes_.data(); }

private:
    static constexpr size_t kNoPlane = ~size_t(0);
    struct Entry {
        Data2D* image;
        Use use;
        size_t bytes;  // 0: a plane of the container's size, kNoPlane: none, else a block of that many bytes
    };
    flow2d_context* context_;
    DataSize3 size_;
    SizeCheck check_;
    std::vector<Entry> entries_;
    std::vector<DevicePtr> planes_;
    bool allocated_ = false;
};
