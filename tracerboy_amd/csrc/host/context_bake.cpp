/* context_bake.cpp -- lightmap baking (include/tracerboy_hip.h tb_bake_lightmap .. tb_run_bake_dilate): a UV atlas rasterised
 * on the device (kernels/bake_kernels.hip), its texels traced by the radiance query as it stands (context_radiance.cpp traceRadianceOnDevice), the
 * sums resolved and the gutters filled.  The atlas's rays, texel records and sums stay in the context (tb_context::Bake) from the first bake to the
 * scene's release; nothing else of the context is written. */
#include "query_call.h"
#include "radiance_trace.h"
#include "../kernels/bake_launch.h"

using namespace tbhost;
using namespace tbctx;

namespace {

typedef tb_context::Bake Bake;

uint32_t numVertices(const tb_context* c) { return (uint32_t)(c->scene.positions.size() / 3); }
DevBuf stagedAtLeast(const void* host, size_t bytes) { DevBuf d = scratch(std::max<size_t>(16, bytes)); if (bytes) HIP_TRY(hipMemcpy(d.p, host, bytes, hipMemcpyHostToDevice)); return d; }

/* The scene's triangles and positions where the rasteriser reads them.  The vertex numbers go up once per Bake (a rebuild releases it with the
 * scene); the positions once per scene generation: from section 21's staged array where it holds exactly what was committed (device to device),
 * else from the host's copy, brought up first if a commit left it stale. */
void bringMesh(tb_context* c, Bake& b)
{
    const HostScene& s = c->scene;
    if (!b.triVerts.p) {
        for (uint32_t v : s.triVertexIndex) if (v >= numVertices(c)) throw std::runtime_error("tb_bake_lightmap: a vertex index of the scene is out of range");
        ensure(b.triVerts, std::max<size_t>(16, s.triVertexIndex.size() * 4));
        if (!s.triVertexIndex.empty()) HIP_TRY(hipMemcpy(b.triVerts.p, s.triVertexIndex.data(), s.triVertexIndex.size() * 4, hipMemcpyHostToDevice));
    }
    if (b.positionsOf == c->sceneGeneration && b.positions.p) return;
    const size_t bytes = s.positions.size() * 4;
    ensure(b.positions, std::max<size_t>(16, bytes));
    const tb_context::Dynamic* d = c->dyn.get();
    if (d && d->ready && d->dirtyPositions.empty() && d->positions.p && d->positions.bytes >= bytes) {
        if (bytes) HIP_TRY(hipMemcpyAsync(b.positions.p, d->positions.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {
        refreshHostScene(c);
        if (bytes) HIP_TRY(hipMemcpy(b.positions.p, c->scene.positions.data(), bytes, hipMemcpyHostToDevice));
    }
    b.positionsOf = c->sceneGeneration;
}

/* resolve + `passes` fill passes on the stream; which of rgba[] holds the picture */
int finish(hipStream_t stream, uint32_t W, uint32_t H, uint32_t passes, const TbBakeTexel* texels, const TbFloat4* sums, DevBuf (&rgba)[2])
{
    HIP_TRY(bake_launch_resolve(stream, (uint64_t)W * H, texels, sums, (TbFloat4*)rgba[0].p));
    int at = 0;
    for (uint32_t p = 1; p <= passes; p++, at ^= 1) HIP_TRY(bake_launch_dilate(stream, W, H, p, (const TbFloat4*)rgba[at].p, (TbFloat4*)rgba[at ^ 1].p));
    return at;
}

} // namespace

extern "C" int tb_bake_lightmap(tb_context* c, const tb_output_settings* settings, float time, const tb_bake_call* call, const float* uv, float* rgbaOut)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        char why[96];
        if (tb_bake_refusal(call, uv, rgbaOut, why, sizeof why) != TB_OK) return fail(c, TB_E_INVALID, std::string("tb_bake_lightmap: ") + why);
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
        if (const int rc = refuseGroup(c, "tb_bake_lightmap", "an atlas is baked on one device")) return rc;
        if (!c->scene.instances.empty()) return fail(c, TB_E_UNSUPPORTED,
            "tb_bake_lightmap: a two-level scene (option flatten_instances = 0 with instances) is not supported: its vertices are in object space");
        const tb_output_settings s = settingsOrDefault(settings);
        if (s.RenderModeRealTime) return fail(c, TB_E_UNSUPPORTED, "tb_bake_lightmap: the real-time mode is not supported: a query has no AOVs and no history");
        const uint32_t W = call->width, H = call->height;
        const size_t n = (size_t)W * H;
        const bool device = (call->flags & TB_BAKE_DEVICE) != 0, accumulate = (call->flags & TB_BAKE_ACCUMULATE) != 0;
        if (device) { /* the arrays go to and from buffers the context keeps, below: only the pointers are the seam's */
            if (uv && !accumulate) checkDevicePointer(c, "tb_bake_lightmap", "uv", uv, 8ull * numVertices(c));
            checkDevicePointer(c, "tb_bake_lightmap", "rgba_out", rgbaOut, 16 * n);
        }
        if (accumulate) {
            const Bake* b = c->bake.get();
            if (!b || !b->held || b->width != W || b->height != H) return fail(c, TB_E_INVALID, "tb_bake_lightmap: TB_BAKE_ACCUMULATE: the context holds no bake of this size");
            if (b->rasterOf != c->sceneGeneration) return fail(c, TB_E_INVALID,
                "tb_bake_lightmap: TB_BAKE_ACCUMULATE: the geometry has been committed since the bake was rasterised");
        }
        if (!c->bake) c->bake.reset(new Bake());
        Bake& b = *c->bake;
        /* from here on the buffers change: a failure below leaves no bake */
        b.held = false;
        ensure(b.rays, sizeof(TbRadianceRay) * n); ensure(b.texels, sizeof(TbBakeTexel) * n); ensure(b.sums, 16 * n);
        ensure(b.rgba[0], 16 * n); ensure(b.rgba[1], 16 * n); ensure(b.covered, 256);
        b.width = W; b.height = H;
        HIP_TRY(hipEventRecord(b.ev[0].create(), c->stream));
        if (!accumulate) {
            bringMesh(c, b);
            DevBuf hostUv; if (uv && !device) hostUv = stagedAtLeast(uv, 8ull * numVertices(c));
            BakeMesh mesh{};
            mesh.positions = (const float*)b.positions.p; mesh.triVerts = (const uint32_t*)b.triVerts.p;
            mesh.normals = (const float*)c->ds.vertexBuffer; mesh.normalStride = 8; /* TbVertex: Normal at float 0, UV at float 3 */
            if (uv) { mesh.uv = device ? uv : (const float*)hostUv.p; mesh.uvStride = 2; }
            else { mesh.uv = (const float*)c->ds.vertexBuffer + 3; mesh.uvStride = 8; }
            mesh.numTris = (uint32_t)(c->scene.triVertexIndex.size() / 3); mesh.numVertices = numVertices(c);
            if ((size_t)mesh.numVertices * 8 > c->scene.vertexBuffer.size()) throw std::runtime_error("tb_bake_lightmap: the scene has fewer vertex records than positions");
            ensure(b.scratch, bake_raster_scratch_bytes(mesh.numTris, W, H));
            HIP_TRY(bake_launch_raster(c->stream, &mesh, W, H, b.scratch.p, b.scratch.bytes, (TbRadianceRay*)b.rays.p, (TbBakeTexel*)b.texels.p, (uint32_t*)b.covered.p));
            HIP_TRY(hipEventRecord(b.ev[1].create(), c->stream));
            HIP_TRY(hipMemcpyAsync(&b.lastCovered, b.covered.p, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream)); /* hostUv goes out of scope */
            b.rasterOf = c->sceneGeneration;
        } else HIP_TRY(hipEventRecord(b.ev[1].create(), c->stream));
        const RadCall k{call->first_sample, call->num_samples, 1u, accumulate ? 1u : 0u, 0.0f};
        const int rc = traceRadianceOnDevice(c, "tb_bake_lightmap", s, time, k, n, (const TbRadianceRay*)b.rays.p, (TbFloat4*)b.sums.p);
        if (rc != TB_OK) return rc;
        HIP_TRY(hipEventRecord(b.ev[2].create(), c->stream));
        const int at = finish(c->stream, W, H, call->dilate_passes, (const TbBakeTexel*)b.texels.p, (const TbFloat4*)b.sums.p, b.rgba);
        HIP_TRY(hipEventRecord(b.ev[3].create(), c->stream));
        if (device) HIP_TRY(hipMemcpyAsync(rgbaOut, b.rgba[at].p, 16 * n, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!device) HIP_TRY(hipMemcpy(rgbaOut, b.rgba[at].p, 16 * n, hipMemcpyDeviceToHost));
        b.lastRasterMs = elapsed(b.ev[0], b.ev[1]); b.lastTraceMs = c->rad.lastMs; b.lastFinishMs = elapsed(b.ev[2], b.ev[3]);
        b.held = true;
        return TB_OK;
    });
}

extern "C" int tb_read_bake(tb_context* c, TbRadianceRay* rays, TbBakeTexel* texels, float* sums)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        const Bake* b = c->bake.get();
        if (!b || !b->held) return fail(c, TB_E_INVALID, "tb_read_bake: the context holds no bake");
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(rays, b->rays); copyBack(texels, b->texels); copyBack(sums, b->sums);
        return TB_OK;
    });
}

extern "C" int tb_run_bake_raster(tb_context* c, uint32_t W, uint32_t H, uint32_t numVerts, const float* positions, const float* normals, const float* uvs,
    uint32_t numTris, const uint32_t* triVerts, TbRadianceRay* raysOut, TbBakeTexel* texelsOut)
{
    return guarded(c, [&]() {
        if (W == 0 || H == 0 || W > BAKE_MAX_SIDE || H > BAKE_MAX_SIDE) return fail(c, TB_E_INVALID, "tb_run_bake_raster: a side of the atlas is 0 or above 8192");
        if (!raysOut || !texelsOut || (numVerts && (!positions || !normals || !uvs)) || (numTris && !triVerts)) return fail(c, TB_E_INVALID, "tb_run_bake_raster: null pointer");
        if (numTris > 0x7fffffffu / 3u) return fail(c, TB_E_INVALID, "tb_run_bake_raster: too many triangles");
        for (size_t i = 0; i < 3ull * numTris; i++) if (triVerts[i] >= numVerts) return fail(c, TB_E_INVALID, "tb_run_bake_raster: a vertex number is not below n_vertices");
        const size_t n = (size_t)W * H;
        const DevBuf dPos = stagedAtLeast(positions, 12ull * numVerts), dNrm = stagedAtLeast(normals, 12ull * numVerts), dUv = stagedAtLeast(uvs, 8ull * numVerts),
            dTri = stagedAtLeast(triVerts, 12ull * numTris);
        const DevBuf dRays = scratch(sizeof(TbRadianceRay) * n), dTexels = scratch(sizeof(TbBakeTexel) * n), dCovered = scratch(256),
            dScratch = scratch(bake_raster_scratch_bytes(numTris, W, H));
        BakeMesh mesh{};
        mesh.positions = (const float*)dPos.p; mesh.normals = (const float*)dNrm.p; mesh.normalStride = 3; mesh.uv = (const float*)dUv.p; mesh.uvStride = 2;
        mesh.triVerts = (const uint32_t*)dTri.p; mesh.numTris = numTris; mesh.numVertices = numVerts;
        HIP_TRY(bake_launch_raster(c->stream, &mesh, W, H, dScratch.p, dScratch.bytes, (TbRadianceRay*)dRays.p, (TbBakeTexel*)dTexels.p, (uint32_t*)dCovered.p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(raysOut, dRays); copyBack(texelsOut, dTexels);
        return TB_OK;
    });
}

extern "C" int tb_run_bake_dilate(tb_context* c, uint32_t W, uint32_t H, uint32_t passes, const float* rgbaIn, float* rgbaOut)
{
    return guarded(c, [&]() {
        if (W == 0 || H == 0 || W > BAKE_MAX_SIDE || H > BAKE_MAX_SIDE) return fail(c, TB_E_INVALID, "tb_run_bake_dilate: a side of the picture is 0 or above 8192");
        if (passes > 16u) return fail(c, TB_E_INVALID, "tb_run_bake_dilate: more than 16 passes");
        if (!rgbaIn || !rgbaOut) return fail(c, TB_E_INVALID, "tb_run_bake_dilate: null pointer");
        const size_t bytes = 16ull * W * H;
        DevBuf pingPong[2] = {staged(rgbaIn, bytes), scratch(bytes)};
        int at = 0;
        for (uint32_t p = 1; p <= passes; p++, at ^= 1) HIP_TRY(bake_launch_dilate(c->stream, W, H, p, (const TbFloat4*)pingPong[at].p, (TbFloat4*)pingPong[at ^ 1].p));
        HIP_TRY(hipStreamSynchronize(c->stream));
        copyBack(rgbaOut, pingPong[at]);
        return TB_OK;
    });
}
