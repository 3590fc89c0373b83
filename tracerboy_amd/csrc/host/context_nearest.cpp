/* context_nearest.cpp -- point queries (include/tracerboy_hip.h tb_nearest_points, tb_bake_distance_field): for a caller's
 * points, or the cells of a grid, the nearest point of the scene's triangles by the rule of include/tb_nearest.h, on host arrays (staged by
 * query_call.h's QueryIo) or on device buffers (nothing allocated per call).  Reads the scene; writes nothing of the context but the kernel's time. */
#include "query_call.h"
#include "../kernels/pq_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {

/* What both calls do once their arguments have passed, in tb_trace_rays's order: the scene, nothing to do, the arrays, launch(points, out) between
 * the query's events.  points: null for a field, whose positions are made in the kernel; n: the points or the cells, outBytes: of all of them */
template <class Launch> int run(tb_context* c, const char* who, uint32_t flags, uint64_t n, const TbQueryPoint* points, void* out, size_t outBytes, Launch launch)
{
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    if (c->ds.numInstances) return fail(c, TB_E_UNSUPPORTED, std::string(who) + ": not supported for a two-level scene: an instance transform with non-uniform "
        "scale does not keep nearest points (load with option flatten_instances = 1)");
    if (n == 0) return TB_OK;
    QueryIo io(c, who, (flags & TB_NEAREST_DEVICE) != 0);
    const TbQueryPoint* p = points ? io.in("points", points, (size_t)n * sizeof(TbQueryPoint)) : nullptr;
    void* o = io.out("out", out, outBytes);
    timed(c->stream, c->pq.ev, c->pq.lastMs, [&]() { return launch(p, o); });
    io.finish();
    return TB_OK;
}

} // namespace

extern "C" int tb_nearest_points(tb_context* c, uint32_t flags, uint64_t n, const TbQueryPoint* points, TbNearest* out)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_nearest_points", "a query's points are answered on one device")) return rc;
    return guarded(c, [&]() {
        char why[96];
        if (tb_nearest_refusal(flags, n, points, out, nullptr, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_nearest_points: ") + why);
        return run(c, "tb_nearest_points", flags, n, points, out, (size_t)n * sizeof(TbNearest), [&](const TbQueryPoint* p, void* o) {
            return pq_launch_nearest(c->stream, &c->ds, flags & TB_NEAREST_SIGNED, (uint32_t)n, p, (TbNearest*)o); });
    });
}

extern "C" int tb_bake_distance_field(tb_context* c, uint32_t flags, const tb_probe_grid* grid, float maxDistance, float* out)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_bake_distance_field", "a field is baked on one device")) return rc;
    return guarded(c, [&]() {
        char why[96];
        if (flags & ~(TB_NEAREST_SIGNED | TB_NEAREST_DEVICE)) return fail(c, TB_E_INVALID, "tb_bake_distance_field: unknown flag bits");
        if (!grid) return fail(c, TB_E_INVALID, "tb_bake_distance_field: null grid");
        if (tb_nearest_refusal(flags, 0, nullptr, out, grid, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_bake_distance_field: ") + why);
        const uint64_t cells = (uint64_t)grid->count[0] * grid->count[1] * grid->count[2]; /* not 0: the refusal above */
        return run(c, "tb_bake_distance_field", flags, cells, nullptr, out, (size_t)cells * sizeof(float), [&](const TbQueryPoint*, void* o) {
            return pq_launch_field(c->stream, &c->ds, flags & TB_NEAREST_SIGNED, grid, maxDistance, (float*)o); });
    });
}
