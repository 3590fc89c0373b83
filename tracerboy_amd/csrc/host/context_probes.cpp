/* context_probes.cpp -- light probes (include/tracerboy_hip.h tb_bake_probes .. tb_run_probe_project): around every position
 * the rays of an octahedral map (kernels/probe_kernels.hip), traced by the radiance query and the closest-hit query as they stand
 * (context_radiance.cpp traceRadianceOnDevice, context_rays.cpp traceClosestOnDevice), projected onto nine SH basis functions per probe; and the
 * consumer's half, tb_sample_probes.  The records, and where the call asks for it the rays' answers, stay in the context (tb_context::Probes) from
 * the first bake to the scene's release; nothing else of the context is written. */
#include "query_call.h"
#include "radiance_trace.h"
#include "../kernels/probe_launch.h"

#include <cstdlib>

using namespace tbhost;
using namespace tbctx;

namespace {

typedef tb_context::Probes Probes;

/* TB_PROBE_MAX_RAYS, read at every call: the most rays of one batch, 1 .. 2^26; unset, empty or anything else: 2^20.  A batch is whole probes, at
 * least one.  The split changes no byte of the answer: a ray's answers depend on its record and the samples alone. */
uint64_t maxRaysOfBatch()
{
    const char* e = getenv("TB_PROBE_MAX_RAYS");
    char* end = nullptr;
    const long long v = e && *e ? strtoll(e, &end, 10) : 0;
    return e && *e && !*end && v >= 1 && v <= (1ll << 26) ? (uint64_t)v : (1ull << 20);
}

} // namespace

extern "C" int tb_bake_probes(tb_context* c, const tb_output_settings* settings, float time, const tb_probe_call* call, const float* positions, TbProbe* probesOut)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        char why[96];
        if (tb_probes_refusal(call, positions, probesOut, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_bake_probes: ") + why);
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
        if (const int rc = refuseGroup(c, "tb_bake_probes", "probes are baked on one device")) return rc;
        const tb_output_settings s = settingsOrDefault(settings);
        if (s.RenderModeRealTime) return fail(c, TB_E_UNSUPPORTED, "tb_bake_probes: the real-time mode is not supported: a query has no AOVs and no history");
        const uint64_t n = call->n; const uint32_t M = call->resolution, texels = M * M;
        if (n == 0) return TB_OK;
        const bool device = (call->flags & TB_PROBES_DEVICE) != 0, accumulate = (call->flags & TB_PROBES_ACCUMULATE) != 0;
        const bool keep = accumulate || (call->flags & TB_PROBES_KEEP_MAPS) != 0;
        if (device) { /* the arrays go to and from buffers the context keeps, below: only the pointers are the seam's */
            checkDevicePointer(c, "tb_bake_probes", "positions", positions, 12 * n);
            checkDevicePointer(c, "tb_bake_probes", "probes_out", probesOut, sizeof(TbProbe) * n);
        }
        if (accumulate) {
            const Probes* p = c->probes.get();
            if (!p || !p->held || !p->mapsHeld) return fail(c, TB_E_INVALID, "tb_bake_probes: TB_PROBES_ACCUMULATE: the context holds no bake with its maps (TB_PROBES_KEEP_MAPS)");
            if (p->n != n || p->resolution != M) return fail(c, TB_E_INVALID, "tb_bake_probes: TB_PROBES_ACCUMULATE: the bake held has another number of probes or another resolution");
            if (p->bakedOf != c->sceneGeneration) return fail(c, TB_E_INVALID, "tb_bake_probes: TB_PROBES_ACCUMULATE: the scene has changed since the bake held was traced");
        }
        if (!c->probes) c->probes.reset(new Probes());
        Probes& p = *c->probes;
        /* from here on the buffers change: a failure below leaves no bake */
        p.held = false; p.mapsHeld = false;
        const uint64_t perBatch = std::min<uint64_t>(n, std::max<uint64_t>(1, maxRaysOfBatch() / texels)), batchRays = perBatch * texels, allRays = n * texels;
        ensure(p.radRays, sizeof(TbRadianceRay) * batchRays); ensure(p.queryRays, sizeof(TbQueryRay) * batchRays);
        ensure(p.sums, 16 * (keep ? allRays : batchRays)); ensure(p.hits, sizeof(TbQueryHit) * (keep ? allRays : batchRays));
        ensure(p.records, sizeof(TbProbe) * n);
        const float* where = positions;
        if (!device) { ensure(p.positions, 12 * n); HIP_TRY(hipMemcpy(p.positions.p, positions, 12 * n, hipMemcpyHostToDevice)); where = (const float*)p.positions.p; }
        p.n = n; p.resolution = M; p.bakedOf = c->sceneGeneration; p.lastBatches = 0;
        p.lastRaysMs = p.lastTraceMs = p.lastHitsMs = p.lastProjectMs = 0.0f;
        for (uint64_t b0 = 0; b0 < n; b0 += perBatch) {
            const uint32_t nb = (uint32_t)std::min<uint64_t>(perBatch, n - b0);
            const uint64_t rays = (uint64_t)nb * texels, at = keep ? b0 * texels : 0;
            TbFloat4* sums = (TbFloat4*)p.sums.p + at; TbQueryHit* hits = (TbQueryHit*)p.hits.p + at;
            HIP_TRY(hipEventRecord(p.ev[0].create(), c->stream));
            HIP_TRY(probe_launch_rays(c->stream, where + 3 * b0, nb, M, call->first_probe_number + (uint32_t)b0, (TbRadianceRay*)p.radRays.p, (TbQueryRay*)p.queryRays.p));
            HIP_TRY(hipEventRecord(p.ev[1].create(), c->stream));
            const RadCall k{call->first_sample, call->num_samples, 0u, accumulate ? 1u : 0u, 0.0f};
            const int rc = traceRadianceOnDevice(c, "tb_bake_probes", s, time, k, rays, (const TbRadianceRay*)p.radRays.p, sums);
            if (rc != TB_OK) return rc;
            HIP_TRY(hipEventRecord(p.ev[2].create(), c->stream));
            traceClosestOnDevice(c, (uint32_t)rays, (const TbQueryRay*)p.queryRays.p, hits);
            HIP_TRY(hipEventRecord(p.ev[3].create(), c->stream));
            HIP_TRY(probe_launch_project(c->stream, where + 3 * b0, nb, M, sums, hits, (TbProbe*)p.records.p + b0));
            HIP_TRY(hipEventRecord(p.ev[4].create(), c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            p.lastRaysMs += elapsed(p.ev[0], p.ev[1]); p.lastTraceMs += c->rad.lastMs; p.lastHitsMs += elapsed(p.ev[2], p.ev[3]); p.lastProjectMs += elapsed(p.ev[3], p.ev[4]);
            p.lastBatches++;
        }
        HIP_TRY(hipMemcpy(probesOut, p.records.p, sizeof(TbProbe) * n, device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
        HIP_TRY(hipStreamSynchronize(c->stream));
        p.held = true; p.mapsHeld = keep;
        return TB_OK;
    });
}

extern "C" int tb_read_probe_maps(tb_context* c, float* sums, TbQueryHit* hits)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        const Probes* p = c->probes.get();
        if (!p || !p->held || !p->mapsHeld) return fail(c, TB_E_INVALID, "tb_read_probe_maps: the context holds no bake with its maps (TB_PROBES_KEEP_MAPS)");
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(sums, p->sums); copyBack(hits, p->hits);
        return TB_OK;
    });
}

extern "C" int tb_sample_probes(tb_context* c, uint32_t flags, const tb_probe_grid* grid, uint32_t resolution, float backfaceLimit, const TbProbe* probes,
    uint64_t n, const float* points, const float* normals, float* rgbaOut)
{
    return guarded(c, [&]() {
        if (flags & ~TB_PROBES_DEVICE) return fail(c, TB_E_INVALID, "tb_sample_probes: unknown flag bits");
        if (!grid) return fail(c, TB_E_INVALID, "tb_sample_probes: null grid");
        if (resolution < PROBE_MIN_RES || resolution > PROBE_MAX_RES) return fail(c, TB_E_INVALID, "tb_sample_probes: the resolution is outside [2, 64]");
        if (!grid->count[0] || !grid->count[1] || !grid->count[2]) return fail(c, TB_E_INVALID, "tb_sample_probes: a count of the grid is 0");
        const uint64_t numProbes = (uint64_t)grid->count[0] * grid->count[1] * grid->count[2];
        if (grid->count[0] > (1u << 24) || grid->count[1] > (1u << 24) || numProbes > (1ull << 24)) return fail(c, TB_E_INVALID, "tb_sample_probes: more than 2^24 probes");
        if (backfaceLimit != backfaceLimit) return fail(c, TB_E_INVALID, "tb_sample_probes: backface_limit is a NaN");
        if (n > (1ull << 31)) return fail(c, TB_E_INVALID, "tb_sample_probes: more than 2^31 points");
        if (!probes || (n && (!points || !normals || !rgbaOut))) return fail(c, TB_E_INVALID, "tb_sample_probes: null pointer");
        const bool device = (flags & TB_PROBES_DEVICE) != 0;
        if (device && (((uintptr_t)probes & 15u) || ((uintptr_t)rgbaOut & 15u) || ((uintptr_t)points & 3u) || ((uintptr_t)normals & 3u)))
            return fail(c, TB_E_INVALID, "tb_sample_probes: device probes and rgba_out are 16-B, points and normals 4-B aligned");
        if (n == 0 && !device) return TB_OK; /* nothing to stage; device probes are checked all the same */
        QueryIo io(c, "tb_sample_probes", device);
        const TbProbe* records = io.in("probes", probes, sizeof(TbProbe) * numProbes);
        if (n == 0) return TB_OK;
        const float* p = io.in("points", points, 12 * n);
        const float* nrm = io.in("normals", normals, 12 * n);
        TbFloat4* o = (TbFloat4*)io.out("rgba_out", rgbaOut, 16 * n);
        HIP_TRY(probe_launch_sample(c->stream, grid, resolution, backfaceLimit, records, (uint32_t)n, p, nrm, o));
        HIP_TRY(hipStreamSynchronize(c->stream));
        io.finish();
        return TB_OK;
    });
}

extern "C" int tb_run_probe_rays(tb_context* c, uint32_t n, uint32_t M, uint32_t firstNumber, const float* positions, TbRadianceRay* radianceOut, TbQueryRay* queryOut)
{
    return guarded(c, [&]() {
        if (M < PROBE_MIN_RES || M > PROBE_MAX_RES) return fail(c, TB_E_INVALID, "tb_run_probe_rays: the resolution is outside [2, 64]");
        if (n == 0 || (uint64_t)n * M * M > (1ull << 24)) return fail(c, TB_E_INVALID, "tb_run_probe_rays: no probes, or more than 2^24 rays");
        if (!positions || !radianceOut || !queryOut) return fail(c, TB_E_INVALID, "tb_run_probe_rays: null pointer");
        const size_t rays = (size_t)n * M * M;
        const DevBuf dPos = staged(positions, 12ull * n), dRad = scratch(sizeof(TbRadianceRay) * rays), dQuery = scratch(sizeof(TbQueryRay) * rays);
        HIP_TRY(probe_launch_rays(c->stream, (const float*)dPos.p, n, M, firstNumber, (TbRadianceRay*)dRad.p, (TbQueryRay*)dQuery.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(radianceOut, dRad); copyBack(queryOut, dQuery);
        return TB_OK;
    });
}

extern "C" int tb_run_probe_project(tb_context* c, uint32_t n, uint32_t M, const float* positions, const float* sums, const TbQueryHit* hits, TbProbe* probesOut)
{
    return guarded(c, [&]() {
        if (M < PROBE_MIN_RES || M > PROBE_MAX_RES) return fail(c, TB_E_INVALID, "tb_run_probe_project: the resolution is outside [2, 64]");
        if (n == 0 || (uint64_t)n * M * M > (1ull << 24)) return fail(c, TB_E_INVALID, "tb_run_probe_project: no probes, or more than 2^24 rays");
        if (!positions || !sums || !hits || !probesOut) return fail(c, TB_E_INVALID, "tb_run_probe_project: null pointer");
        const size_t rays = (size_t)n * M * M;
        const DevBuf dPos = staged(positions, 12ull * n), dSums = staged(sums, 16 * rays), dHits = staged(hits, sizeof(TbQueryHit) * rays), dOut = scratch(sizeof(TbProbe) * n);
        HIP_TRY(probe_launch_project(c->stream, (const float*)dPos.p, n, M, (const TbFloat4*)dSums.p, (const TbQueryHit*)dHits.p, (TbProbe*)dOut.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(probesOut, dOut);
        return TB_OK;
    });
}
