/* context_meshes.cpp -- a scene from caller arrays (include/tracerboy_hip.h tb_load_meshes): the argument tests, device arrays
 * read to the host once, the scene made by host_scene.cpp MeshesToScene into a local HostScene, then the swap and finalizeScene -- what a file load
 * does from there on.  A refused call has not touched the context's scene. */
#include "query_call.h"

using namespace tbhost;
using namespace tbctx;

namespace {

/* the arrays of TB_MESH_DEVICE meshes on the host: each checked as section 20 checks its pointers, then copied on the context's stream */
struct HostCopies { std::vector<std::vector<float>> floats; std::vector<std::vector<uint32_t>> words; std::vector<tb_mesh_desc> meshes; };

std::string readDeviceMeshes(tb_context* c, const tb_scene_desc& desc, HostCopies& h)
{
    h.meshes.assign(desc.meshes, desc.meshes + desc.n_meshes);
    for (uint32_t m = 0; m < desc.n_meshes; m++) {
        const tb_mesh_desc& d = desc.meshes[m];
        struct { const char* name; const void* p; size_t bytes; } arrays[4] = {{"positions", d.positions, 12ull * d.n_vertices},
            {"indices", d.indices, 12ull * d.n_triangles}, {"normals", d.normals_or_null, 12ull * d.n_vertices}, {"uvs", d.uvs_or_null, 8ull * d.n_vertices}};
        for (const auto& a : arrays) if (a.p) if (const char* why = devicePointerRefusal(c, a.p, a.bytes))
            return "mesh " + std::to_string(m) + ": " + a.name + ": " + why;
    }
    for (uint32_t m = 0; m < desc.n_meshes; m++) {
        tb_mesh_desc& d = h.meshes[m];
        auto floatsOf = [&](const float* p, size_t n) -> const float* {
            if (!p) return nullptr;
            h.floats.emplace_back(n);
            HIP_TRY(hipMemcpyAsync(h.floats.back().data(), p, n * 4, hipMemcpyDeviceToHost, c->stream));
            return h.floats.back().data();
        };
        d.positions = floatsOf(d.positions, 3ull * d.n_vertices);
        d.normals_or_null = floatsOf(d.normals_or_null, 3ull * d.n_vertices);
        d.uvs_or_null = floatsOf(d.uvs_or_null, 2ull * d.n_vertices);
        h.words.emplace_back(3ull * d.n_triangles);
        HIP_TRY(hipMemcpyAsync(h.words.back().data(), d.indices, 12ull * d.n_triangles, hipMemcpyDeviceToHost, c->stream));
        d.indices = h.words.back().data();
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return std::string();
}

} // namespace

extern "C" int tb_load_meshes(tb_context* c, const tb_scene_desc* desc)
{
    TB_REFUSE_PEER(c);
    return guarded(c, [&]() {
        { const std::string no = MeshesRefusal(desc); if (!no.empty()) return fail(c, TB_E_INVALID, "tb_load_meshes: " + no); }
        if (!c->group.peers.empty()) return fail(c, TB_E_UNSUPPORTED, "tb_load_meshes: not supported for a multi-device group");
        { const std::string no = MeshesUnsupported(*desc); if (!no.empty()) return fail(c, TB_E_UNSUPPORTED, "tb_load_meshes: " + no); }
        tb_scene_desc host = *desc;
        HostCopies copies;
        if (desc->flags & TB_MESH_DEVICE) {
            const std::string no = readDeviceMeshes(c, *desc, copies);
            if (!no.empty()) return fail(c, TB_E_INVALID, "tb_load_meshes: " + no);
            host.meshes = copies.meshes.data(); host.flags &= ~TB_MESH_DEVICE;
        }
        HostScene local; std::string why;
        const int rc = MeshesToScene(host, local, why);
        if (rc != TB_OK) return fail(c, rc, "tb_load_meshes: " + why);
        HIP_TRY(hipStreamSynchronize(c->stream)); /* nothing in flight reads the scene that goes */
        c->hasScene = false;
        c->scene = std::move(local);
        finalizeScene(c);
        return TB_OK;
    });
}
