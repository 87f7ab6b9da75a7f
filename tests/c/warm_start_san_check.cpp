// What a sanitizer can see of the warm start without a device: the adaptive rule (OpticalFlow2D::WarmNextReach), the options check
// (OpticalFlow2D::WarmOptionsOk), the start-level rule it feeds, and the refusals of flow2d_propagate_flow_2d, which all come before
// the entry touches its context.  Built by `make -C cuda-flow2d_amd/host san_warm` with AddressSanitizer + UBSan; exits 0 when every
// check holds.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "flow2d_c_abi.h"
#include "optical_flow_2d.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            ++failures;                                                 \
        }                                                               \
    } while (0)

int main()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // ---- the adaptive rule
    struct Case {
        unsigned long long count, above[3];
        float tail;
        int used;
        bool redo;
        int next;
    };
    const Case cases[] = {
        {1000, {50, 10, 0}, 0.05f, 0, false, 1},  {1000, {51, 50, 0}, 0.05f, 0, false, 2},   {1000, {400, 51, 50}, 0.05f, 0, false, 3},
        {1000, {900, 800, 51}, 0.05f, 0, false, 0}, {0, {0, 0, 0}, 0.05f, 0, false, 0},      {0, {0, 0, 0}, 0.05f, 2, true, 0},
        {1000, {400, 51, 50}, 0.05f, 1, true, 3}, {1000, {400, 51, 50}, 0.05f, 2, true, 3},  {1000, {400, 51, 50}, 0.05f, 3, false, 3},
        {1000, {900, 800, 51}, 0.05f, 3, true, 0}, {1000, {0, 0, 0}, 0.f, 1, false, 1},      {~0ull, {~0ull, ~0ull, ~0ull}, 0.5f, 3, true, 0},
    };
    for (const Case& c : cases) {
        bool redo = !c.redo;
        int next = -1;
        CHECK(OpticalFlow2D::WarmNextReach(c.count, c.above, c.tail, c.used, &redo, &next));
        CHECK(redo == c.redo && next == c.next);
    }
    {
        const unsigned long long good[3] = {50, 10, 0}, rising[3] = {50, 60, 0}, beyond[3] = {2000, 10, 0};
        bool redo = false;
        int next = 77;
        CHECK(!OpticalFlow2D::WarmNextReach(1000, nullptr, 0.05f, 0, &redo, &next));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, good, 0.05f, 0, nullptr, &next));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, good, 0.05f, 0, &redo, nullptr));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, good, 1.f, 0, &redo, &next));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, good, -0.5f, 0, &redo, &next));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, good, nan, 0, &redo, &next));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, good, 0.05f, 4, &redo, &next));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, good, 0.05f, -1, &redo, &next));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, rising, 0.05f, 0, &redo, &next));
        CHECK(!OpticalFlow2D::WarmNextReach(1000, beyond, 0.05f, 0, &redo, &next));
        CHECK(next == 77);  // a refused call writes nothing
    }
    // ---- the options
    {
        OpticalFlow2D::WarmOptions o;
        CHECK(OpticalFlow2D::WarmOptionsOk(o));
        o.tail = 0.f;
        CHECK(OpticalFlow2D::WarmOptionsOk(o));
        for (float tail : {1.f, 2.f, nan, inf}) {
            o = OpticalFlow2D::WarmOptions();
            o.tail = tail;
            CHECK(!OpticalFlow2D::WarmOptionsOk(o));
        }
        for (int fill : {-1, FLOW2D_PROPAGATE_MAX_FILL + 1}) {
            o = OpticalFlow2D::WarmOptions();
            o.fill_passes = fill;
            CHECK(!OpticalFlow2D::WarmOptionsOk(o));
        }
        for (float scale : {-1.f, nan, inf}) {
            o = OpticalFlow2D::WarmOptions();
            o.photo_scale = scale;
            CHECK(!OpticalFlow2D::WarmOptionsOk(o));
        }
        // the reaches of the rule through the start-level rule
        size_t start = 99;
        CHECK(OpticalFlow2D::PriorStartLevel(4096, 4096, 50, 0.9f, 1.f, -1, &start) && start == 0);
        CHECK(OpticalFlow2D::PriorStartLevel(4096, 4096, 50, 0.9f, 2.f, -1, &start) && start == 7);
        CHECK(OpticalFlow2D::PriorStartLevel(4096, 4096, 50, 0.9f, 3.f, -1, &start) && start == 11);
    }
    // ---- the entry's refusals: made-up addresses, nothing is dereferenced before the device is entered
    {
        std::vector<char> fake(4096);
        flow2d_context* ctx = reinterpret_cast<flow2d_context*>(fake.data());
        const size_t w = 96, h = 80, pitch = 512, span = pitch * h, work = flow2d_propagate_flow_workspace_bytes(w, h, 1);
        CHECK(work == w * h * 16 && flow2d_propagate_flow_workspace_bytes(0, h, 1) == 0);
        auto at = [&](size_t k) { return reinterpret_cast<float*>((size_t(1) << 20) + k * (span + 4096)); };
        auto rec = reinterpret_cast<unsigned long long*>(at(7));
        auto call = [&](flow2d_context* c, float* u, float* mask, float* f0, float* f1, size_t ww, size_t hh, size_t p, float step,
                        float photo, int fill, float* ou, unsigned long long* record, void* workspace) {
            return flow2d_propagate_flow_2d(c, u, at(1), mask, f0, f1, ww, hh, p, step, photo, fill, ou, at(6), record, workspace);
        };
        const int bad = FLOW2D_ERR_INVALID_ARGUMENT;
        CHECK(call(nullptr, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, 4, at(5), rec, at(8)) == bad);
        CHECK(call(ctx, nullptr, at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, 4, at(5), rec, at(8)) == bad);
        CHECK(call(ctx, at(0), at(2), at(3), at(4), 0, h, pitch, 1.f, 1.f, 4, at(5), rec, at(8)) == bad);
        CHECK(call(ctx, at(0), at(2), at(3), at(4), 70000, 70000, 280000, 1.f, 1.f, 4, at(5), rec, at(8)) == bad);
        CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch + 8, 1.f, 1.f, 4, at(5), rec, at(8)) == bad);
        CHECK(call(ctx, at(0), at(2), nullptr, at(4), w, h, pitch, 1.f, 1.f, 4, at(5), rec, at(8)) == bad);
        CHECK(call(ctx, at(0), at(2), at(3), nullptr, w, h, pitch, 1.f, 1.f, 4, at(5), rec, at(8)) == bad);
        for (float step : {0.f, nan, inf}) CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, step, 1.f, 4, at(5), rec, at(8)) == bad);
        for (float photo : {-1.f, nan, inf}) CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, photo, 4, at(5), rec, at(8)) == bad);
        for (int fill : {-1, 65}) CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, fill, at(5), rec, at(8)) == bad);
        CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, 4, at(5), rec, nullptr) == bad);
        CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, 4, at(5), rec, reinterpret_cast<char*>(at(8)) + 8) == bad);
        CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, 4, at(5), reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(at(7)) + 4), at(8)) == bad);
        CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, 4, at(0), rec, at(8)) == bad);      // out_u is flow_u
        CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, 4, at(5), rec, at(1)) == bad);      // the workspace meets flow_v
        CHECK(call(ctx, at(0), at(2), at(3), at(4), w, h, pitch, 1.f, 1.f, 4, at(5), reinterpret_cast<unsigned long long*>(at(5)) + 1, at(8)) == bad);
    }
    std::printf(failures ? "warm_start_san_check: %d check(s) FAILED\n" : "warm_start_san_check: all checks hold\n", failures);
    return failures ? 1 : 0;
}
