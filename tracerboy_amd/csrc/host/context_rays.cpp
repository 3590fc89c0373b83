/* context_rays.cpp -- ray queries (include/tracerboy_hip.h tb_trace_rays): a caller's rays through the traversal the renderer
 * uses, closest-hit records or occlusion flags out, on host arrays (staged by query_call.h's QueryIo) or on device buffers (nothing allocated per call).
 * Reads the scene; writes nothing of the context but the work counter of the any-hit walk's refilling form. */
#include "query_call.h"
#include "../kernels/rq_launch.h"

#include <cstdlib>

using namespace tbhost;
using namespace tbctx;

namespace {

/* why tb_trace_rays refuses its arguments; null: it does not.  (What needs the context -- a scene, a group -- is asked there.) */
const char* raysRefusal(uint32_t modeAndFlags, uint64_t n, const void* rays, const void* out)
{
    if (modeAndFlags & ~(0xffu | TB_RAYS_DEVICE)) return "unknown flag bits";
    const uint32_t mode = modeAndFlags & 0xffu;
    if (mode != TB_RAYS_CLOSEST && mode != TB_RAYS_OCCLUDED) return "unknown mode";
    if (n > (1ull << 31)) return "more than 2^31 rays";
    if (n && (!rays || !out)) return "null pointer";
    if (n && (modeAndFlags & TB_RAYS_DEVICE)) {
        if ((uintptr_t)rays & 15u) return "device rays are not 16-B aligned";
        if (mode == TB_RAYS_CLOSEST && ((uintptr_t)out & 15u)) return "device hit records are not 16-B aligned";
    }
    return nullptr;
}

/* Diagnostics of scripts/ray_query_rate.py, which measures the forms of occluded mode against each other in one process: TB_RQ_REFILL = 1 .. 64, the
 * refilling any-hit walk with that many idle lanes per refill; 0, the any-hit walk with one ray per lane; -1, the closest-hit walk and t < TMax.
 * Unset, empty or anything else (-2 here): what ships, rq_refill_for. */
int refillDiagnostic()
{
    const char* e = getenv("TB_RQ_REFILL");
    const int v = e && *e ? atoi(e) : -2;
    return v >= -1 && v <= 64 ? v : -2;
}

} // namespace

void tbctx::traceClosestOnDevice(tb_context* c, uint32_t n, const TbQueryRay* rays, TbQueryHit* hits)
{
    HIP_TRY(rq_launch_closest(c->stream, &c->ds, n, rays, hits, nullptr));
}

extern "C" int tb_trace_rays(tb_context* c, uint32_t modeAndFlags, uint64_t n, const TbQueryRay* rays, void* out)
{
    TB_REFUSE_PEER(c);
    if (const int rc = refuseGroup(c, "tb_trace_rays", "a query's rays are traced on one device")) return rc;
    return guarded(c, [&]() {
        if (const char* why = raysRefusal(modeAndFlags, n, rays, out)) return fail(c, TB_E_INVALID, std::string("tb_trace_rays: ") + why);
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
        if (n == 0) return TB_OK;
        const bool closest = (modeAndFlags & 0xffu) == TB_RAYS_CLOSEST;
        QueryIo io(c, "tb_trace_rays", (modeAndFlags & TB_RAYS_DEVICE) != 0);
        const TbQueryRay* r = io.in("rays", rays, (size_t)n * sizeof(TbQueryRay));
        void* o = io.out("out", out, closest ? (size_t)n * sizeof(TbQueryHit) : (size_t)n);
        const int diag = closest ? -2 : refillDiagnostic();
        if (closest) traceClosestOnDevice(c, (uint32_t)n, r, (TbQueryHit*)o);
        else if (c->ds.numInstances || diag == -1) HIP_TRY(rq_launch_closest(c->stream, &c->ds, (uint32_t)n, r, nullptr, (uint8_t*)o));
        else {
            const uint32_t refill = diag >= 0 ? (uint32_t)diag : rq_refill_for(c->ds.numTris);
            if (refill && !c->rq.counter.p) ensure(c->rq.counter, 64);
            HIP_TRY(rq_launch_occluded(c->stream, &c->ds, (uint32_t)n, r, (uint8_t*)o, (uint32_t*)c->rq.counter.p, refill));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        io.finish();
        return TB_OK;
    });
}
