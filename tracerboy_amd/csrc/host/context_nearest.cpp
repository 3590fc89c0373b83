/* context_nearest.cpp -- point queries (include/tracerboy_hip.h tb_nearest_points, tb_bake_distance_field): for a caller's
 * points, or the cells of a grid, the nearest point of the scene's triangles by the rule of include/tb_nearest.h, on host arrays (staged like the
 * test hooks) or on device buffers (nothing allocated per call).  Reads the scene; writes nothing of the context but the kernel's time. */
#include "context_internal.h"
#include "../kernels/pq_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {

/* what both calls ask of the context once their arguments have passed, in tb_trace_rays's order; TB_OK: go on */
int sceneRefusal(tb_context* c, const char* who)
{
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    if (c->ds.numInstances) return fail(c, TB_E_UNSUPPORTED, std::string(who) + ": not supported for a two-level scene: an instance transform with non-uniform "
        "scale does not keep nearest points (load with option flatten_instances = 1)");
    return TB_OK;
}

template <class Launch> void timedLaunch(tb_context* c, Launch launch)
{
    HIP_TRY(hipEventRecord(c->pq.ev[0].create(), c->stream));
    HIP_TRY(launch());
    HIP_TRY(hipEventRecord(c->pq.ev[1].create(), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->pq.lastMs, c->pq.ev[0], c->pq.ev[1]));
}

} // namespace

extern "C" int tb_nearest_points(tb_context* c, uint32_t flags, uint64_t n, const TbQueryPoint* points, TbNearest* out)
{
    TB_REFUSE_PEER(c);
    if (c && !c->group.peers.empty()) return fail(c, TB_E_UNSUPPORTED,
        "tb_nearest_points: not supported for a multi-device group: a query's points are answered on one device");
    return guarded(c, [&]() {
        char why[96];
        if (tb_nearest_refusal(flags, n, points, out, nullptr, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_nearest_points: ") + why);
        if (const int rc = sceneRefusal(c, "tb_nearest_points")) return rc;
        if (n == 0) return TB_OK;
        const bool device = (flags & TB_NEAREST_DEVICE) != 0;
        const size_t pointBytes = (size_t)n * sizeof(TbQueryPoint), outBytes = (size_t)n * sizeof(TbNearest);
        DevBuf dPoints, dOut; /* the host path's staging: temporary, like tb_trace_rays's */
        if (device) {
            if (const char* no = devicePointerRefusal(c, points, pointBytes)) return fail(c, TB_E_INVALID, std::string("tb_nearest_points: points: ") + no);
            if (const char* no = devicePointerRefusal(c, out, outBytes)) return fail(c, TB_E_INVALID, std::string("tb_nearest_points: out: ") + no);
        } else { dPoints = staged(points, pointBytes); dOut = scratch(outBytes); }
        const TbQueryPoint* p = device ? points : (const TbQueryPoint*)dPoints.p;
        TbNearest* o = device ? out : (TbNearest*)dOut.p;
        timedLaunch(c, [&]() { return pq_launch_nearest(c->stream, &c->ds, flags & TB_NEAREST_SIGNED, (uint32_t)n, p, o); });
        if (!device) copyBack(out, dOut);
        return TB_OK;
    });
}

extern "C" int tb_bake_distance_field(tb_context* c, uint32_t flags, const tb_probe_grid* grid, float maxDistance, float* out)
{
    TB_REFUSE_PEER(c);
    if (c && !c->group.peers.empty()) return fail(c, TB_E_UNSUPPORTED,
        "tb_bake_distance_field: not supported for a multi-device group: a field is baked on one device");
    return guarded(c, [&]() {
        char why[96];
        if (flags & ~(TB_NEAREST_SIGNED | TB_NEAREST_DEVICE)) return fail(c, TB_E_INVALID, "tb_bake_distance_field: unknown flag bits");
        if (!grid) return fail(c, TB_E_INVALID, "tb_bake_distance_field: null grid");
        if (tb_nearest_refusal(flags, 0, nullptr, out, grid, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_bake_distance_field: ") + why);
        if (const int rc = sceneRefusal(c, "tb_bake_distance_field")) return rc;
        const bool device = (flags & TB_NEAREST_DEVICE) != 0;
        const size_t outBytes = (size_t)grid->count[0] * grid->count[1] * grid->count[2] * sizeof(float);
        DevBuf dOut;
        if (device) { if (const char* no = devicePointerRefusal(c, out, outBytes)) return fail(c, TB_E_INVALID, std::string("tb_bake_distance_field: out: ") + no); }
        else dOut = scratch(outBytes);
        float* o = device ? out : (float*)dOut.p;
        timedLaunch(c, [&]() { return pq_launch_field(c->stream, &c->ds, flags & TB_NEAREST_SIGNED, grid, maxDistance, o); });
        if (!device) copyBack(out, dOut);
        return TB_OK;
    });
}
