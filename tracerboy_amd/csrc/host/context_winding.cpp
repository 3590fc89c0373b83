/* context_winding.cpp -- winding numbers (include/tracerboy_hip.h tb_winding_numbers, tb_bake_winding_field,
 * tb_nearest_points_winding, tb_bake_distance_field_winding): robust inside / outside by the rule of include/tb_winding.h, on host arrays (staged
 * by query_call.h's QueryIo) or on device buffers.  The subtree moments belong to the scene: made lazily, fitted again after a commit, released with
 * the scene.  Reads the scene; writes nothing of the context but them and the kernels' times. */
#include "query_call.h"
#include "winding_host.h"
#include "../kernels/pq_launch.h"
#include "../kernels/refit_launch.h"
#include "../kernels/wn_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {

typedef tb_context::Winding Winding;
const char* const kOneDevice = "a query's points are answered on one device";

int sceneRefusal(tb_context* c, const char* who)
{
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    if (c->ds.numInstances) return fail(c, TB_E_UNSUPPORTED, std::string(who) + ": not supported for a two-level scene (load with option flatten_instances = 1)");
    /* a pre-split triangle lies in the tree once per reference, and a sum over the leaves would count it as often (the refit refuses the same trees) */
    if (c->scene.trisB.size() != c->scene.triGeometry.size()) return fail(c, TB_E_UNSUPPORTED, std::string(who) +
        ": not supported for a tree of pre-split references (option presplit): its leaves hold a triangle more than once");
    return TB_OK;
}

/* the moments of the tree as the device holds it now: the tables once per topology, the fit once per scene generation */
Winding& momentsOf(tb_context* c)
{
    if (!c->wn) c->wn.reset(new Winding());
    Winding& w = *c->wn;
    if (!w.tablesReady) {
        std::vector<uint32_t> triSlot, nodeSlot, schedule;
        treeSchedule(c->scene, triSlot, nodeSlot, schedule, w.levelFirst);
        if (triSlot.size() != c->ds.numTris || nodeSlot.size() != c->ds.numNodes) throw std::runtime_error("winding numbers: the host's tree is not the device's");
        uploadInto(c, w.triSlot, triSlot); uploadInto(c, w.nodeSlot, nodeSlot); uploadInto(c, w.schedule, schedule); uploadInto(c, w.levelFirstDevice, w.levelFirst);
        ensure(w.moments, std::max<size_t>(64, (size_t)c->ds.numNodes * sizeof(TbMomentsB)));
        ensure(w.areas, std::max<size_t>(16, (size_t)c->ds.numNodes * 8));
        ensure(w.root, 32);
        HIP_TRY(hipStreamSynchronize(c->stream)); /* the vectors above go out of scope */
        w.tablesReady = true;
    }
    if (!w.fitted || w.fittedOf != c->sceneGeneration) {
        WnTables t{};
        t.triSlot = (const uint32_t*)w.triSlot.p; t.nodeSlot = (const uint32_t*)w.nodeSlot.p; t.schedule = (const uint32_t*)w.schedule.p;
        t.tris = c->ds.tris; t.nodes = c->ds.nodes; t.moments = (TbMomentsB*)w.moments.p; t.areas = (float*)w.areas.p; t.root = (float*)w.root.p;
        t.numTris = c->ds.numTris; t.numNodes = c->ds.numNodes;
        const uint32_t numLevels = (uint32_t)w.levelFirst.size() - 1;
        timed(c->stream, w.evFit, w.lastFitMs, [&]() { return wn_launch_fit(c->stream, &t, w.levelFirst.data(), numLevels, (const uint32_t*)w.levelFirstDevice.p,
            refit_fused_first_level(w.levelFirst.data(), numLevels)); });
        w.fitted = true; w.fittedOf = c->sceneGeneration;
    }
    return w;
}

/* What the four calls do once their arguments and the scene have passed and there is something to do: the arrays, the moments, launch(w, points, out)
 * between the walk's events.  points: null for a field, whose positions are made in the kernel; n: the points or the cells, outBytes: of all of them */
template <class Launch> int run(tb_context* c, const char* who, bool device, uint64_t n, const TbQueryPoint* points, void* out, size_t outBytes, Launch launch)
{
    QueryIo io(c, who, device);
    const TbQueryPoint* p = points ? io.in("points", points, (size_t)n * sizeof(TbQueryPoint)) : nullptr;
    void* o = io.out("out", out, outBytes);
    Winding& w = momentsOf(c);
    timed(c->stream, w.ev, w.lastMs, [&]() { return launch(w, p, o); });
    io.finish();
    return TB_OK;
}

hipError_t walkPoints(tb_context* c, const Winding& w, int mode, uint64_t n, const TbQueryPoint* p, float beta, void* o)
{
    return wn_launch_points(c->stream, &c->ds, (const TbMomentsB*)w.moments.p, (const float*)w.root.p, mode, (uint32_t)n, p, beta, o);
}

hipError_t walkGrid(tb_context* c, const Winding& w, int mode, const tb_probe_grid* grid, float beta, void* o)
{
    return wn_launch_grid(c->stream, &c->ds, (const TbMomentsB*)w.moments.p, (const float*)w.root.p, mode, grid, beta, (float*)o);
}

uint64_t numCells(const tb_probe_grid* grid) { return (uint64_t)grid->count[0] * grid->count[1] * grid->count[2]; }

} // namespace

extern "C" int tb_winding_numbers(tb_context* c, uint32_t flags, uint64_t n, const TbQueryPoint* points, float beta, float* out)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_winding_numbers", kOneDevice)) return rc;
    return guarded(c, [&]() {
        char why[96];
        if (tb_winding_refusal(flags, n, points, out, nullptr, beta, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_winding_numbers: ") + why);
        if (const int rc = sceneRefusal(c, "tb_winding_numbers")) return rc;
        if (n == 0) return TB_OK;
        if (flags & TB_WINDING_HOST_WALK) { /* the kernel's walk over the host copies of what the device holds */
            refreshHostScene(c);
            const HostScene& s = c->scene;
            const tbwinding::Tree tree{s.nodesB.data(), s.nodesB.size(), s.trisB.data(), s.trisB.size(), s.rootRefB};
            tbwinding::run(tree, true, n, points, beta, out);
            return TB_OK;
        }
        return run(c, "tb_winding_numbers", (flags & TB_WINDING_DEVICE) != 0, n, points, out, (size_t)n * sizeof(float),
            [&](const Winding& w, const TbQueryPoint* p, void* o) { return walkPoints(c, w, WN_WRITE, n, p, beta, o); });
    });
}

extern "C" int tb_bake_winding_field(tb_context* c, uint32_t flags, const tb_probe_grid* grid, float beta, float* out)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_bake_winding_field", kOneDevice)) return rc;
    return guarded(c, [&]() {
        char why[96];
        if (flags & ~TB_WINDING_DEVICE) return fail(c, TB_E_INVALID, "tb_bake_winding_field: unknown flag bits");
        if (!grid) return fail(c, TB_E_INVALID, "tb_bake_winding_field: null grid");
        if (tb_winding_refusal(flags, 0, nullptr, out, grid, beta, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_bake_winding_field: ") + why);
        if (const int rc = sceneRefusal(c, "tb_bake_winding_field")) return rc;
        return run(c, "tb_bake_winding_field", (flags & TB_WINDING_DEVICE) != 0, numCells(grid), nullptr, out, (size_t)numCells(grid) * sizeof(float),
            [&](const Winding& w, const TbQueryPoint*, void* o) { return walkGrid(c, w, WN_WRITE, grid, beta, o); });
    });
}

extern "C" int tb_nearest_points_winding(tb_context* c, uint32_t flags, uint64_t n, const TbQueryPoint* points, float beta, TbNearest* out)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_nearest_points_winding", kOneDevice)) return rc;
    return guarded(c, [&]() {
        char why[96];
        if (flags & ~TB_NEAREST_DEVICE) return fail(c, TB_E_INVALID, "tb_nearest_points_winding: unknown flag bits (TB_NEAREST_SIGNED is the other rule's)");
        if (tb_nearest_refusal(flags, n, points, out, nullptr, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_nearest_points_winding: ") + why);
        if (!(beta >= 1.0f)) return fail(c, TB_E_INVALID, "tb_nearest_points_winding: beta is a NaN or below 1");
        if (const int rc = sceneRefusal(c, "tb_nearest_points_winding")) return rc;
        if (n == 0) return TB_OK;
        return run(c, "tb_nearest_points_winding", (flags & TB_NEAREST_DEVICE) != 0, n, points, out, (size_t)n * sizeof(TbNearest),
            [&](const Winding& w, const TbQueryPoint* p, void* o) { /* the unsigned query, unchanged, then the sign pass: chained on the stream */
                const hipError_t e = pq_launch_nearest(c->stream, &c->ds, 0u, (uint32_t)n, p, (TbNearest*)o);
                return e != hipSuccess ? e : walkPoints(c, w, WN_SIGN_RECORDS, n, p, beta, o);
            });
    });
}

extern "C" int tb_bake_distance_field_winding(tb_context* c, uint32_t flags, const tb_probe_grid* grid, float maxDistance, float beta, float* out)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_bake_distance_field_winding", kOneDevice)) return rc;
    return guarded(c, [&]() {
        char why[96];
        if (flags & ~TB_NEAREST_DEVICE) return fail(c, TB_E_INVALID, "tb_bake_distance_field_winding: unknown flag bits (TB_NEAREST_SIGNED is the other rule's)");
        if (!grid) return fail(c, TB_E_INVALID, "tb_bake_distance_field_winding: null grid");
        if (tb_nearest_refusal(flags, 0, nullptr, out, grid, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_bake_distance_field_winding: ") + why);
        if (!(beta >= 1.0f)) return fail(c, TB_E_INVALID, "tb_bake_distance_field_winding: beta is a NaN or below 1");
        if (const int rc = sceneRefusal(c, "tb_bake_distance_field_winding")) return rc;
        return run(c, "tb_bake_distance_field_winding", (flags & TB_NEAREST_DEVICE) != 0, numCells(grid), nullptr, out, (size_t)numCells(grid) * sizeof(float),
            [&](const Winding& w, const TbQueryPoint*, void* o) {
                const hipError_t e = pq_launch_field(c->stream, &c->ds, 0u, grid, maxDistance, (float*)o);
                return e != hipSuccess ? e : walkGrid(c, w, WN_SIGN_CELLS, grid, beta, o);
            });
    });
}
