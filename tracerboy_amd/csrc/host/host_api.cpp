/* host_api.cpp -- the entry points of include/tracerboy_hip.h that need no device: host scenes (tb_host_scene_*), the scene view and digest, image
 * files, the launch plan as a pure function, frame groups, the host un-permute of gathered tiles.  Includes no HIP header and not the context's
 * internal header: it compiles with a plain C++ compiler (tests/test_abi.py); what it shares with the context's files is in host_shared.h. */
#include "host_shared.h"
#include "launch_plan.h"
#include "lds_image.h"
#include "options.h"
#include "tb_state.h"
#include "wave_cost.h"
#include "../kernels/probe_launch.h"
#include "tb_nearest.h"
#include "winding_host.h"

#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <thread>

using namespace tbhost;
using namespace tbctx;

void tbctx::fillSceneInfo(const HostScene& s, tb_scene_info* o)
{
    memset(o, 0, sizeof *o);
    o->numTriangles = (uint32_t)s.triGeometry.size(); o->numVertices = (uint32_t)(s.positions.size() / 3); o->numMaterials = (uint32_t)s.materials.size();
    o->numLights = (uint32_t)s.lights.size(); o->numGeometries = (uint32_t)s.hitGroups.size(); o->numTextures = (uint32_t)s.textureData.size();
    o->bvhBytesA = (uint32_t)s.bvhA.size(); o->bvhNodesB = (uint32_t)s.nodesB.size(); o->bvhMaxDepth = s.bvhMaxDepth;
    o->filmWidth = (uint32_t)s.filmWidth; o->filmHeight = (uint32_t)s.filmHeight;
    memcpy(o->sceneMin, s.sceneMin, 12); memcpy(o->sceneMax, s.sceneMax, 12);
}

void tbctx::fillView(const HostScene& s, TbSceneView* v)
{
    memset(v, 0, sizeof *v);
    v->bvh = s.bvhA.data(); v->bvhBytes = (uint32_t)s.bvhA.size(); v->numTriangles = (uint32_t)s.triGeometry.size();
    v->hitGroups = s.hitGroups.data(); v->numHitGroups = (uint32_t)s.hitGroups.size();
    v->indexBuffer = s.indexBuffer.data(); v->numIndices = (uint32_t)s.indexBuffer.size();
    v->vertexBuffer = s.vertexBuffer.data(); v->numVertexFloats = (uint32_t)s.vertexBuffer.size();
    v->materials = s.materials.data(); v->numMaterials = (uint32_t)s.materials.size();
    v->textureData = s.textureData.empty() ? nullptr : s.textureData.data(); v->numTextureData = (uint32_t)s.textureData.size();
    v->lights = s.lights.empty() ? nullptr : s.lights.data(); v->numLights = (uint32_t)s.lights.size();
    v->images = s.images.empty() ? nullptr : s.images.data(); v->numImages = (uint32_t)s.images.size();
    v->texelPool = s.texelPool.empty() ? nullptr : s.texelPool.data();
    v->envMap = s.envMap.empty() ? nullptr : s.envMap.data(); v->envWidth = s.envWidth; v->envHeight = s.envHeight;
    v->blueNoise0 = s.blueNoise0.empty() ? nullptr : s.blueNoise0.data(); v->blueNoise1 = s.blueNoise1.empty() ? nullptr : s.blueNoise1.data();
    v->config = s.config;
    if (!s.instances.empty()) { v->tlas = s.tlasA.data(); v->tlasBytes = (uint32_t)s.tlasA.size(); v->numInstances = (uint32_t)s.instances.size(); }
    v->numBlas = s.blasOffsets.empty() ? 0u : (uint32_t)s.blasOffsets.size() - 1u; v->blasOffsets = s.blasOffsets.empty() ? nullptr : s.blasOffsets.data();
}

/* The scene digest (include/tb_state.h): every array of the kernel seam, each prefixed by its length.  The camera's lens height, which
 * tb_set_camera writes into the config constants, is left out: the camera travels with a render state on its own. */
uint64_t tbctx::sceneDigestOf(const HostScene& s)
{
    TbSceneView v; fillView(s, &v);
    TbStateDigest d{0, 0};
    tb_state_digest_array(&d, v.bvh, v.bvhBytes);
    tb_state_digest_array(&d, v.hitGroups, (uint64_t)v.numHitGroups * sizeof(TbHitGroupRecord));
    tb_state_digest_array(&d, v.indexBuffer, (uint64_t)v.numIndices * 4u);
    tb_state_digest_array(&d, v.vertexBuffer, (uint64_t)v.numVertexFloats * 4u);
    tb_state_digest_array(&d, v.materials, (uint64_t)v.numMaterials * sizeof(TbMaterial));
    tb_state_digest_array(&d, v.textureData, (uint64_t)v.numTextureData * sizeof(TbTextureData));
    tb_state_digest_array(&d, v.lights, (uint64_t)v.numLights * sizeof(TbLight));
    tb_state_digest_array(&d, v.images, (uint64_t)v.numImages * sizeof(TbImageDesc));
    tb_state_digest_array(&d, v.texelPool, (uint64_t)s.texelPool.size() * sizeof(TbFloat4));
    tb_state_digest_array(&d, v.envMap, (uint64_t)v.envWidth * v.envHeight * sizeof(TbFloat4));
    TbConfigConstants config = v.config; config.CameraLensHeight = 0.0f;
    tb_state_digest_array(&d, &config, sizeof config);
    tb_state_digest_array(&d, v.tlas, v.tlasBytes);
    tb_state_digest_array(&d, v.blasOffsets, v.blasOffsets ? ((uint64_t)v.numBlas + 1u) * 4u : 0u);
    return d.sum;
}

extern "C" {

static bool hasSuffix(const char* path, const char* suf) { size_t n = strlen(path), m = strlen(suf); return n >= m && strcmp(path + n - m, suf) == 0; }
int tb_write_image_rgba8(const char* path, uint32_t W, uint32_t H, const uint8_t* rgba8)
{
    if (!path || !rgba8 || !W || !H) return TB_E_INVALID;
    if (!hasSuffix(path, ".png")) return TB_E_UNSUPPORTED;
    std::string err;
    return tbhost::WritePngRGBA8(path, W, H, rgba8, err) ? TB_OK : TB_E_IO;
}
int tb_write_image_f32(const char* path, uint32_t W, uint32_t H, const float* rgba)
{
    if (!path || !rgba || !W || !H) return TB_E_INVALID;
    std::string err;
    if (hasSuffix(path, ".exr")) return tbhost::WriteExrRGBA(path, W, H, rgba, err) ? TB_OK : TB_E_IO;
    if (!hasSuffix(path, ".pfm")) return TB_E_UNSUPPORTED;
    return tbhost::WritePfmRGB(path, W, H, rgba, err) ? TB_OK : TB_E_IO;
}

int tb_decode_image(const char* path, uint32_t* W, uint32_t* H, int* normalized, int* hasAlpha, float* rgba)
{
    if (!path || !W || !H) return TB_E_INVALID;
    try {
        std::vector<TbFloat4> texels; bool norm = false, alpha = false; std::string err;
        if (!tbhost::LoadImageRGBA32F(path, texels, *W, *H, norm, err, &alpha)) { g_createError = err; return TB_E_IO; }
        if (normalized) *normalized = norm; if (hasAlpha) *hasAlpha = alpha;
        if (rgba) memcpy(rgba, texels.data(), texels.size() * sizeof(TbFloat4));
        return TB_OK;
    } catch (const std::exception& e) { g_createError = e.what(); return TB_E_IO; }
}

void tb_plan_defaults(tb_plan_input* in)
{
    if (!in) return;
    memset(in, 0, sizeof *in);
    in->high_occupancy = OptionDefault(OPT_high_occupancy); in->stack_overflow_max = OptionDefault(OPT_stack_overflow_max);
    in->primary_prepass = OptionDefault(OPT_primary_prepass); in->overlap_launches = OptionDefault(OPT_overlap_launches);
    in->pooled_samples = OptionDefault(OPT_pooled_samples); in->costly_first = (uint32_t)OptionDefault(OPT_costly_first);
    in->split_trav = OptionDefault(OPT_split_trav); in->guided_groups = OptionDefault(OPT_guided_groups);
}

uint32_t tb_frame_groups(uint32_t frames, uint32_t frameGroup, uint32_t guided, uint32_t group, uint32_t* firstFrame, uint32_t* numFrames)
{
    uint32_t lg = 0; while ((2u << lg) <= frameGroup) lg++;
    const uint32_t total = tb_fg_groups(frames, lg, guided ? 1u : 0u, 0xffffffffu, nullptr, nullptr);
    if (group < total) { uint32_t f0 = 0, l = 0; (void)tb_fg_groups(frames, lg, guided ? 1u : 0u, group, &f0, &l);
        if (firstFrame) *firstFrame = f0; if (numFrames) *numFrames = std::min(1u << l, frames - std::min(frames, f0)); }
    return total;
}

int tb_plan_launch(const tb_plan_input* in, tb_launch_plan* out)
{
    if (!in || !out || !in->width || !in->height) return TB_E_INVALID;
    PlanLaunch(*in, *out);
    return TB_OK;
}

/* Why tb_trace_radiance refuses its arguments before it looks at the context or allocates anything: pure tests, in the order
 * the header lists them.  What needs the context -- a scene, a group, real-time settings, whose memory a device pointer is -- is asked there. */
static const char* radianceRefusal(const TbRadianceCall* call, uint64_t n, const void* rays, const void* out)
{
    if (!call) return "null call";
    if (call->mode_and_flags & ~(0xffu | TB_RADIANCE_DEVICE | TB_RADIANCE_ACCUMULATE)) return "unknown flag bits";
    const uint32_t mode = call->mode_and_flags & 0xffu;
    if (mode != TB_RADIANCE_RAY && mode != TB_RADIANCE_HEMISPHERE) return "unknown mode";
    if (call->num_samples == 0) return "num_samples is 0";
    if (call->num_samples > (1u << 24)) return "more than 2^24 samples per ray";
    if ((uint64_t)call->first_sample + call->num_samples > (1ull << 32)) return "first_sample + num_samples passes 2^32";
    if (!(call->seed_advance - call->seed_advance == 0.0f)) return "seed_advance is not finite";
    if (n > (1ull << 31)) return "more than 2^31 rays";
    if (n && (!rays || !out)) return "null pointer";
    if (n && (call->mode_and_flags & TB_RADIANCE_DEVICE) && ((((uintptr_t)rays) | ((uintptr_t)out)) & 15u)) return "device arrays are not 16-B aligned";
    return nullptr;
}

int tb_radiance_refusal(const TbRadianceCall* call, uint64_t n, const void* rays, const void* out, char* why, uint32_t whyBytes)
{
    const char* no = radianceRefusal(call, n, rays, out);
    if (why && whyBytes) { strncpy(why, no ? no : "", whyBytes - 1); why[whyBytes - 1] = 0; }
    return no ? TB_E_INVALID : TB_OK;
}

/* Why tb_bake_lightmap refuses its arguments before it looks at the context: pure tests, in the order the header lists them. */
static const char* bakeRefusal(const tb_bake_call* call, const void* uv, const void* rgbaOut)
{
    if (!call) return "null call";
    if (call->width == 0 || call->height == 0) return "a side of the atlas is 0";
    if (call->width > 8192u || call->height > 8192u) return "a side of the atlas is above 8192";
    if (call->flags & ~(TB_BAKE_DEVICE | TB_BAKE_ACCUMULATE)) return "unknown flag bits";
    if (call->num_samples == 0) return "num_samples is 0";
    if (call->num_samples > (1u << 24)) return "more than 2^24 samples per texel";
    if ((uint64_t)call->first_sample + call->num_samples > (1ull << 32)) return "first_sample + num_samples passes 2^32";
    if (call->dilate_passes > 16u) return "more than 16 dilate passes";
    if (!rgbaOut) return "null rgba_out";
    if (call->flags & TB_BAKE_DEVICE) {
        if ((uintptr_t)rgbaOut & 15u) return "the device picture is not 16-B aligned";
        if ((uintptr_t)uv & 3u) return "the device UVs are not 4-B aligned";
    }
    return nullptr;
}

int tb_bake_refusal(const tb_bake_call* call, const void* uv, const void* rgbaOut, char* why, uint32_t whyBytes)
{
    const char* no = bakeRefusal(call, uv, rgbaOut);
    if (why && whyBytes) { strncpy(why, no ? no : "", whyBytes - 1); why[whyBytes - 1] = 0; }
    return no ? TB_E_INVALID : TB_OK;
}

/* Why tb_bake_probes refuses its arguments before it looks at the context: pure tests, in the order the header lists them. */
static const char* probesRefusal(const tb_probe_call* call, const void* positions, const void* probesOut)
{
    if (!call) return "null call";
    if (call->resolution < PROBE_MIN_RES || call->resolution > PROBE_MAX_RES) return "the resolution is outside [2, 64]";
    if ((uint64_t)call->n * call->resolution * call->resolution > (1ull << 31)) return "more than 2^31 rays";
    if (call->n > (1u << 24) || (uint64_t)call->first_probe_number + call->n > (1ull << 24)) return "probe numbers above 2^24: the seed is not an exact float";
    if (call->num_samples == 0) return "num_samples is 0";
    if (call->num_samples > (1u << 24)) return "more than 2^24 samples per ray";
    if ((uint64_t)call->first_sample + call->num_samples > (1ull << 32)) return "first_sample + num_samples passes 2^32";
    if (call->flags & ~(TB_PROBES_DEVICE | TB_PROBES_ACCUMULATE | TB_PROBES_KEEP_MAPS)) return "unknown flag bits";
    if (call->n && (!positions || !probesOut)) return "null pointer";
    if (call->n && (call->flags & TB_PROBES_DEVICE)) {
        if ((uintptr_t)positions & 3u) return "the device positions are not 4-B aligned";
        if ((uintptr_t)probesOut & 15u) return "the device probe records are not 16-B aligned";
    }
    return nullptr;
}

int tb_probes_refusal(const tb_probe_call* call, const void* positions, const void* probesOut, char* why, uint32_t whyBytes)
{
    const char* no = probesRefusal(call, positions, probesOut);
    if (why && whyBytes) { strncpy(why, no ? no : "", whyBytes - 1); why[whyBytes - 1] = 0; }
    return no ? TB_E_INVALID : TB_OK;
}

int tb_sh9_irradiance(const TbProbe* probe, const float* normal, float* rgbOut)
{
    if (!probe || !normal || !rgbOut) return TB_E_INVALID;
    float Y[9];
    probe_basis(normal[0], normal[1], normal[2], Y);
    for (int ch = 0; ch < 3; ch++) rgbOut[ch] = probe_sh9_channel(probe->SH + ch, 3, Y);
    return TB_OK;
}

int tb_probe_directions(uint32_t M, float* dirsOut, float* weightsOut)
{
    if (M < PROBE_MIN_RES || M > PROBE_MAX_RES) return TB_E_INVALID;
    for (uint32_t t = 0; t < M * M; t++) {
        float d[3], w;
        probe_direction(M, t % M, t / M, d, &w);
        if (dirsOut) memcpy(dirsOut + 3ull * t, d, 12);
        if (weightsOut) weightsOut[t] = w;
    }
    return TB_OK;
}

int tb_unpack_gathered_host(uint32_t W, uint32_t H, uint32_t world, uint32_t tw, uint32_t th, const float* const* perRank, float* full)
{
    if (!perRank || !full || world == 0 || tw == 0 || th == 0) return TB_E_INVALID;
    uint32_t tilesX = (W + tw - 1) / tw, tilesY = (H + th - 1) / th;
    for (uint32_t t = 0; t < tilesX * tilesY; t++) {
        uint32_t rank = t % world, local = t / world;
        const float* src = perRank[rank] + (size_t)local * tw * th * 4;
        uint32_t x0 = (t % tilesX) * tw, y0 = (t / tilesX) * th;
        uint32_t w = (W - x0 < tw) ? W - x0 : tw, h = (H - y0 < th) ? H - y0 : th;
        for (uint32_t y = 0; y < h; y++) memcpy(full + ((size_t)(y0 + y) * W + x0) * 4, src + (size_t)y * w * 4, (size_t)w * 16);
    }
    return TB_OK;
}

/* ---- host-only scene API ---------------------------------------------------------------------- */
struct tb_host_scene { HostScene scene; };

static int hostFail(char* err, uint32_t n, int code, const std::string& m) { if (err && n) { strncpy(err, m.c_str(), n - 1); err[n - 1] = 0; } return code; }

/* bvh_builder of the host-scene entry points: builder (bits 0-5) | (wave_tree + 1) << 6 | (reinsertion passes + 1) << 8 | reinsertion share (percent) << 16 |
 * presplit (percent, <= 127) << 24; a zero field = the library's own choice (options "wave_tree" / "reinsertion_passes" / "reinsertion_share" of a context) */
static int builderOfWord(int word) { return word & 0x3f; }
static void applyBuilderWord(HostScene& s, int word)
{
    const int wave = (word >> 6) & 3, passes = (word >> 8) & 0xff, share = (word >> 16) & 0xff, presplit = (word >> 24) & 0x7f;
    if (wave) s.waveTree = wave == 1 ? 0 : 1;
    if (passes) s.reinsertionPasses = passes - 1;
    if (share) s.reinsertionShare = share;
    if (presplit) s.presplitPercent = presplit;
}

/* the tree of a built one-level scene, read back from its layout-A image, as wave_cost.h walks it */
static bool waveTreeOfScene(const HostScene& s, WaveTree& w)
{
    if (!s.instances.empty() || s.bvhA.size() < 16) return false;
    uint32_t hdr[4]; memcpy(hdr, s.bvhA.data(), 16);
    const uint32_t N = (uint32_t)s.trisB.size();
    if (!N || (uint64_t)hdr[0] + 32ull * (2ull * N - 1) > s.bvhA.size() || (uint64_t)hdr[1] + 40ull * N > s.bvhA.size()) return false;
    const TbAabbNode* nodes = (const TbAabbNode*)(s.bvhA.data() + hdr[0]);
    w.N = N; w.center.resize(2 * N - 1); w.half.resize(2 * N - 1); w.left.assign(N - 1, 0); w.right.assign(N - 1, 0);
    w.v0.resize(N); w.v1.resize(N); w.v2.resize(N);
    for (uint32_t i = 0; i < 2 * N - 1; i++) {
        w.center[i] = tb3_make(nodes[i].center[0], nodes[i].center[1], nodes[i].center[2]);
        w.half[i] = tb3_make(nodes[i].halfDim[0], nodes[i].halfDim[1], nodes[i].halfDim[2]);
        if (i < N - 1) { w.left[i] = nodes[i].flags & TB_BVH_INDEX_MASK; w.right[i] = nodes[i].rightNodeIndex;
            if (w.left[i] >= 2 * N - 1 || w.right[i] >= 2 * N - 1) return false; }
    }
    for (uint32_t k = 0; k < N; k++) { /* leaf N-1+k holds triangle k of the image (its index field is k) */
        float v[9]; memcpy(v, s.bvhA.data() + hdr[1] + 40ull * k + 4, 36);
        w.v0[k] = tb3_make(v[0], v[1], v[2]); w.v1[k] = tb3_make(v[3], v[4], v[5]); w.v2[k] = tb3_make(v[6], v[7], v[8]);
    }
    return true;
}

int tb_host_scene_load(const char* path, int builder, int loadFlags, tb_host_scene** out, char* err, uint32_t errLen)
{
    if (!path || !out) return TB_E_INVALID;
    *out = nullptr;
    try {
        std::shared_ptr<PbrtScene> ps = importScene(path);
        tb_host_scene* h = new tb_host_scene();
        ConvertOptions co; co.flattenInstances = (loadFlags & 1) != 0; co.flipTextureUVs = (loadFlags & 2) == 0;
        try { ConvertScene(*ps, h->scene, co); applyBuilderWord(h->scene, builder); BuildBvh(h->scene, builderOfWord(builder)); } catch (...) { delete h; throw; }
        *out = h; return TB_OK;
    } catch (const std::exception& e) {
        std::string m = e.what();
        int code = (m.find("open") != std::string::npos || m.find("Couldn't") != std::string::npos) ? TB_E_IO : TB_E_PARSE;
        if (m.find("not supported") != std::string::npos || m.find("unsupported") != std::string::npos) code = TB_E_UNSUPPORTED;
        return hostFail(err, errLen, code, m);
    }
}

int tb_host_scene_procedural(int kind, uint32_t tris, uint32_t seed, int builder, tb_host_scene** out, char* err, uint32_t errLen)
{
    if (!out) return TB_E_INVALID;
    *out = nullptr;
    try {
        tb_host_scene* h = new tb_host_scene();
        try { MakeProceduralScene(h->scene, kind, tris, seed); applyBuilderWord(h->scene, builder); BuildBvh(h->scene, builderOfWord(builder)); } catch (...) { delete h; throw; }
        *out = h; return TB_OK;
    } catch (const std::exception& e) { return hostFail(err, errLen, TB_E_INVALID, e.what()); }
}

/* Why tb_load_meshes refuses its arguments before it looks at the context or reads a value: pure tests, in the header's order. */
int tb_meshes_refusal(const tb_scene_desc* desc, char* why, uint32_t whyBytes)
{
    const std::string no = MeshesRefusal(desc);
    if (why && whyBytes) { strncpy(why, no.c_str(), whyBytes - 1); why[whyBytes - 1] = 0; }
    return no.empty() ? TB_OK : TB_E_INVALID;
}

int tb_host_scene_from_meshes(const tb_scene_desc* desc, int builder, tb_host_scene** out, char* err, uint32_t errLen)
{
    if (!out) return TB_E_INVALID;
    *out = nullptr;
    try {
        { const std::string no = MeshesRefusal(desc); if (!no.empty()) return hostFail(err, errLen, TB_E_INVALID, "tb_host_scene_from_meshes: " + no); }
        if (desc->flags & TB_MESH_DEVICE) return hostFail(err, errLen, TB_E_INVALID, "tb_host_scene_from_meshes: host arrays only (TB_MESH_DEVICE needs a context)");
        std::unique_ptr<tb_host_scene> h(new tb_host_scene());
        std::string why;
        const int rc = MeshesToScene(*desc, h->scene, why);
        if (rc != TB_OK) return hostFail(err, errLen, rc, "tb_host_scene_from_meshes: " + why);
        applyBuilderWord(h->scene, builder); BuildBvh(h->scene, builderOfWord(builder));
        *out = h.release(); return TB_OK;
    } catch (const std::exception& e) { return hostFail(err, errLen, TB_E_INVALID, e.what()); }
}

int tb_host_smooth_normals(const float* positions, uint32_t nv, const uint32_t* indices, uint32_t nt, float* normalsOut)
{
    if ((nv && (!positions || !normalsOut)) || (nt && !indices)) return TB_E_INVALID;
    for (uint64_t i = 0; i < 3ull * nt; i++) if (indices[i] >= nv) return TB_E_INVALID;
    try { SmoothNormals(positions, nv, indices, nt, normalsOut); } catch (const std::exception&) { return TB_E_INVALID; }
    return TB_OK;
}

void tb_host_scene_free(tb_host_scene* s) { delete s; }

int tb_host_scene_view_get(tb_host_scene* s, TbSceneView* v) { if (!s || !v) return TB_E_INVALID; fillView(s->scene, v); return TB_OK; }
int tb_host_scene_digest(tb_host_scene* s, uint64_t* out) { if (!s || !out) return TB_E_INVALID; *out = sceneDigestOf(s->scene); return TB_OK; }
int tb_host_scene_camera(tb_host_scene* s, tb_camera* cam) { if (!s || !cam) return TB_E_INVALID; *cam = s->scene.camera; return TB_OK; }
int tb_host_scene_info(tb_host_scene* h, tb_scene_info* o)
{
    if (!h || !o) return TB_E_INVALID;
    fillSceneInfo(h->scene, o);
    return TB_OK;
}
int tb_host_scene_frame_constants(tb_host_scene* h, const tb_output_settings* settings, uint32_t frame, float t, TbPerFrameConstants* out)
{
    if (!h || !out) return TB_E_INVALID;
    tb_output_settings s; if (settings) s = *settings; else DefaultOutputSettings(s);
    MakeFrameConstants(h->scene, h->scene.camera, s, frame, t, 0xffffffffu, 0xffffffffu, *out);
    return TB_OK;
}
int tb_host_scene_layout_b(tb_host_scene* h, const TbNodeB** nodes, uint32_t* nn, const TbTriB** tris, uint32_t* nt, uint32_t* root)
{
    if (!h) return TB_E_INVALID;
    if (nodes) *nodes = h->scene.nodesB.data(); if (nn) *nn = (uint32_t)h->scene.nodesB.size();
    if (tris) *tris = h->scene.trisB.data(); if (nt) *nt = (uint32_t)h->scene.trisB.size();
    if (root) *root = h->scene.rootRefB;
    return TB_OK;
}
int tb_host_scene_lds_image(tb_host_scene* h, uint8_t* out, uint32_t capacity, tb_lds_image_info* info)
{
    if (!h || !info) return TB_E_INVALID;
    const HostScene& s = h->scene;
    memset(info, 0, sizeof *info);
    const size_t bytes = LdsImageBytes(s.nodesB.size(), s.trisB.size());
    if (bytes > 0x7fffffffull) return TB_E_UNSUPPORTED;
    info->bytes = (uint32_t)bytes; info->num_nodes = (uint32_t)s.nodesB.size(); info->num_tris = (uint32_t)s.trisB.size();
    info->node_stride = TB_LDS_NODE_STRIDE; info->tri_copies = TB_LDS_TRI_COPIES; info->root_ref = s.rootRefB;
    info->stack_depth = WalkStackDepth(s.bvhMaxDepth);
    if (!out) return TB_OK;
    if (capacity < bytes) return TB_E_INVALID;
    const LdsImage im = BuildLdsImage(s.nodesB.data(), s.nodesB.size(), s.trisB.data(), s.trisB.size());
    info->off_nodes = im.offNodes; info->off_tris = im.offTris;
    memcpy(out, im.bytes.data(), im.bytes.size());
    return TB_OK;
}
int tb_host_scene_tables_in_range(const TbTriB* tris, uint32_t numTris, const uint32_t* hitGroups, uint32_t numHitGroups, const uint32_t* indices,
    uint32_t numIndices, uint32_t numVertexFloats, uint32_t numMaterials)
{
    if ((numTris && !tris) || (numHitGroups && !hitGroups) || (numIndices && !indices)) return TB_E_INVALID;
    std::vector<TbDevHitGroup> hg(numHitGroups);
    for (uint32_t i = 0; i < numHitGroups; i++) hg[i] = TbDevHitGroup{hitGroups[4 * i], hitGroups[4 * i + 1], hitGroups[4 * i + 2], 0};
    return SceneTablesInRange(tris, numTris, hg.data(), hg.size(), indices, numIndices, numVertexFloats, numMaterials) ? 1 : 0;
}
int tb_host_scene_triangles(tb_host_scene* h, const float** pos, uint32_t* nv, const uint32_t** tvi, const uint32_t** tg, const uint32_t** tp,
    const uint32_t** tf, uint32_t* nt)
{
    if (!h) return TB_E_INVALID;
    const HostScene& s = h->scene;
    if (pos) *pos = s.positions.data(); if (nv) *nv = (uint32_t)(s.positions.size() / 3);
    if (tvi) *tvi = s.triVertexIndex.data(); if (tg) *tg = s.triGeometry.data(); if (tp) *tp = s.triPrimitive.data(); if (tf) *tf = s.triFlags.data();
    if (nt) *nt = (uint32_t)s.triGeometry.size();
    return TB_OK;
}

/* ---- what a wave pays for a tree (wave_cost.h) -------------------------------------------------- */
static void tripsOut(const WaveTrips& w, tb_wave_trips* o)
{
    o->inner_trips = w.inner; o->leaf_trips = w.leaf; o->idle_passes = w.idle; o->inner_active = w.innerActive; o->leaf_active = w.leafActive;
    o->cost = w.cost();
}
int tb_wave_replay(const char* const* steps, uint32_t lanes, uint32_t parkMin, tb_wave_trips* out)
{
    if (!out || lanes > kWaveLanes || (lanes && !steps)) return TB_E_INVALID;
    uint32_t len[kWaveLanes] = {};
    for (uint32_t l = 0; l < lanes; l++) { if (!steps[l]) return TB_E_INVALID; len[l] = (uint32_t)strlen(steps[l]);
        for (uint32_t k = 0; k < len[l]; k++) if (steps[l][k] != 'I' && steps[l][k] != 'L') return TB_E_INVALID; }
    tripsOut(WaveReplay(steps, len, lanes, parkMin), out);
    return TB_OK;
}
int tb_host_scene_wave_walk(tb_host_scene* h, uint32_t n, const float* origins, const float* dirs, const float* tMax, uint32_t* innerSteps,
    uint32_t* leafSteps, char* steps, uint64_t stepsCapacity)
{
    if (!h || (n && (!origins || !dirs))) return TB_E_INVALID;
    WaveTree w; if (!waveTreeOfScene(h->scene, w)) return TB_E_UNSUPPORTED;
    std::vector<char> one; uint64_t used = 0;
    for (uint32_t i = 0; i < n; i++) {
        WaveRay r; r.o = tb3_make(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]); r.d = tb3_make(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
        r.tMax = tMax ? tMax[i] : kWaveMaxT; WaveRayPrepare(r);
        one.clear(); WaveWalk(w, r, one);
        uint32_t in = 0; for (char c : one) in += c == 'I' ? 1u : 0u;
        if (innerSteps) innerSteps[i] = in; if (leafSteps) leafSteps[i] = (uint32_t)one.size() - in;
        if (steps) { /* the strings back to back, each ended by a 0 */
            if (used + one.size() + 1 > stepsCapacity) return TB_E_INVALID;
            if (!one.empty()) memcpy(steps + used, one.data(), one.size());
            used += one.size(); steps[used++] = 0;
        }
    }
    return TB_OK;
}
static bool modelRaysOf(const HostScene& s, uint32_t seed, uint32_t waves, int feelerPercent, std::vector<WaveRay>& rays)
{
    uint32_t dSeed, dWaves, dFeelers, places; WaveStageSize(dSeed, dWaves, dFeelers, places);
    WaveSurfaces surf; WaveSurfacesOf(s, surf);
    WaveModelRays(surf, seed ? seed : dSeed, waves ? waves : dWaves, feelerPercent < 0 ? dFeelers : (uint32_t)std::min(feelerPercent, 100), rays);
    return !rays.empty();
}
int tb_host_scene_wave_rays(tb_host_scene* h, uint32_t seed, uint32_t waves, int feelerPercent, float* origins, float* dirs, float* tMax, uint32_t capacity)
{
    if (!h || waves > (1u << 16)) return TB_E_INVALID;
    std::vector<WaveRay> rays; modelRaysOf(h->scene, seed, waves, feelerPercent, rays);
    if (origins || dirs || tMax) {
        if (capacity < rays.size()) return TB_E_INVALID;
        for (size_t i = 0; i < rays.size(); i++) {
            if (origins) { origins[3 * i] = rays[i].o.x; origins[3 * i + 1] = rays[i].o.y; origins[3 * i + 2] = rays[i].o.z; }
            if (dirs) { dirs[3 * i] = rays[i].d.x; dirs[3 * i + 1] = rays[i].d.y; dirs[3 * i + 2] = rays[i].d.z; }
            if (tMax) tMax[i] = rays[i].tMax;
        }
    }
    return (int)rays.size();
}
int tb_host_scene_wave_cost(tb_host_scene* h, uint32_t seed, uint32_t waves, int feelerPercent, uint32_t parkMin, tb_wave_trips* out)
{
    if (!h || !out || waves > (1u << 16)) return TB_E_INVALID;
    WaveTree w; if (!waveTreeOfScene(h->scene, w)) return TB_E_UNSUPPORTED;
    std::vector<WaveRay> rays; if (!modelRaysOf(h->scene, seed, waves, feelerPercent, rays)) return TB_E_UNSUPPORTED;
    std::vector<char> arena;
    tripsOut(WaveCostOfTree(w, rays, parkMin ? parkMin : kLdsSceneParkMin, arena), out);
    return TB_OK;
}
int tb_host_scene_wave_stage(tb_host_scene* h, tb_wave_stage_info* o)
{
    if (!h || !o) return TB_E_INVALID;
    const HostScene::WaveStageReport& r = h->scene.waveStage;
    memset(o, 0, sizeof *o);
    o->ran = r.ran; o->rays = r.rays; o->seed = r.seed; o->park_min = r.parkMin; o->depth_limit = r.depthLimit; o->moves = r.moves;
    o->evaluations = r.evaluations; o->inner_insts = kWaveInnerInsts; o->leaf_insts = kWaveLeafInsts;
    o->before.inner_trips = r.innerBefore; o->before.leaf_trips = r.leafBefore; o->before.cost = r.costBefore;
    o->after.inner_trips = r.innerAfter; o->after.leaf_trips = r.leafAfter; o->after.cost = r.costAfter;
    o->milliseconds = r.milliseconds;
    o->places_priced = r.placesPriced; o->abandoned = r.abandoned; o->rays_checked = r.raysChecked; o->rays_rewalked = r.raysRewalked; o->cuts_skipped = r.cutsSkipped;
    o->places_screened = r.placesScreened; o->screen_waves = r.screenWaves; o->screen_keep = r.screenKeep; o->threads = r.threads; o->passes = r.passes;
    o->places = r.places; o->validation_rejects = r.validationRejects; o->validation_before = r.validationBefore; o->validation_after = r.validationAfter;
    return TB_OK;
}
int tb_host_scene_wave_search(tb_host_scene* h, uint32_t seed, uint32_t waves, int feelerPercent, uint32_t places, uint32_t keep, int threads, tb_wave_stage_info* out)
{
    if (!h || waves > (1u << 16) || threads < 0) return TB_E_INVALID;
    HostScene& s = h->scene;
    if (!s.instances.empty() || s.triGeometry.empty()) return TB_E_UNSUPPORTED;
    s.waveTree = 1; s.waveSearchSeed = seed; s.waveSearchWaves = waves; s.waveSearchFeelerPercent = feelerPercent; s.waveSearchPlaces = places; s.waveSearchKeep = keep;
    s.waveTreeThreads = threads;
    try { BuildBvh(s, 1); } catch (const std::exception&) { return TB_E_INVALID; }
    return out ? tb_host_scene_wave_stage(h, out) : TB_OK;
}

/* ---- point queries on the host (the rule: include/tb_nearest.h) ------------- */
/* Why tb_nearest_points (grid null) or tb_bake_distance_field refuses its arguments before it looks at the context: pure tests, in the header's order. */
static const char* nearestRefusal(uint32_t flags, uint64_t n, const void* points, const void* out, const tb_probe_grid* grid, bool isGrid)
{
    if (flags & ~(TB_NEAREST_SIGNED | TB_NEAREST_DEVICE)) return "unknown flag bits";
    if (!isGrid) {
        if (n > (1ull << 31)) return "more than 2^31 points";
        if (n && (!points || !out)) return "null pointer";
        if (n && (flags & TB_NEAREST_DEVICE)) {
            if ((uintptr_t)points & 15u) return "device points are not 16-B aligned";
            if ((uintptr_t)out & 15u) return "device records are not 16-B aligned";
        }
        return nullptr;
    }
    if (!grid) return "null grid";
    if (!grid->count[0] || !grid->count[1] || !grid->count[2]) return "a count of the grid is 0";
    if ((uint64_t)grid->count[0] * grid->count[1] > (1ull << 31) || (uint64_t)grid->count[0] * grid->count[1] * grid->count[2] > (1ull << 31))
        return "more than 2^31 cells";
    for (int k = 0; k < 3; k++) if (!(tb_abs(grid->origin[k]) < tb_u2f(0x7f800000u)) || !(tb_abs(grid->spacing[k]) < tb_u2f(0x7f800000u)))
        return "the grid's origin or spacing is not finite";
    if (!out) return "null pointer";
    if ((flags & TB_NEAREST_DEVICE) && ((uintptr_t)out & 3u)) return "the device distances are not 4-B aligned";
    return nullptr;
}

int tb_nearest_refusal(uint32_t flags, uint64_t n, const void* points, const void* out, const tb_probe_grid* grid, char* why, uint32_t whyBytes)
{
    const char* no = nearestRefusal(flags, n, points, out, grid, grid != nullptr);
    if (why && whyBytes) { strncpy(why, no ? no : "", whyBytes - 1); why[whyBytes - 1] = 0; }
    return no ? TB_E_INVALID : TB_OK;
}

namespace {

struct NearestBest { float d2 = tb_u2f(0x7f800000u); uint32_t geom = TB_NEAREST_NONE, prim = TB_NEAREST_NONE; float u = 0.0f, v = 0.0f; tb3 point{0.0f, 0.0f, 0.0f};
    bool behind = false; };

tb3 cornerOf(const float* v) { return tb3_make(v[0], v[1], v[2]); }

/* the candidate rule on one triangle; true: it is the best now */
bool nearestOffer(NearestBest& best, tb3 p, float limit, const TbTriB& t)
{
    const tb3 v0 = cornerOf(t.v0), v1 = cornerOf(t.v1), v2 = cornerOf(t.v2);
    const TbNearestOnTriangle r = tb_nearest_on_triangle(p, v0, v1, v2);
    if (!(r.D2 <= limit) || !tb_nearest_better(r.D2, t.geometryIndex, t.primitiveIndex, best.d2, best.geom, best.prim)) return false;
    best.d2 = r.D2; best.geom = t.geometryIndex; best.prim = t.primitiveIndex; best.u = r.U; best.v = r.V; best.point = r.Point;
    best.behind = tb_nearest_behind(p, r.Point, v0, v1, v2);
    return true;
}

TbNearest nearestRecord(const NearestBest& best, bool isSigned)
{
    TbNearest o; memset(&o, 0, sizeof o);
    o.Distance = tb_u2f(0x7f800000u); o.Prim = o.Geom = TB_NEAREST_NONE;
    if (best.geom == TB_NEAREST_NONE && best.prim == TB_NEAREST_NONE) return o;
    const float d = tb_sqrt(best.d2);
    o.Point[0] = best.point.x; o.Point[1] = best.point.y; o.Point[2] = best.point.z;
    o.Distance = isSigned && best.behind ? -d : d; o.U = best.u; o.V = best.v; o.Prim = best.prim; o.Geom = best.geom;
    return o;
}

void rootBoxOf(const HostScene& s, tb3& c, tb3& h)
{
    const TbAabbNode* root = (const TbAabbNode*)(s.bvhA.data() + 16);
    c = cornerOf(root->center); h = cornerOf(root->halfDim);
}
tb3 childCentre(const TbNodeB& n, int k) { return tb3_make(n.cx[k], n.cy[k], n.cz[k]); }
tb3 childHalf(const TbNodeB& n, int k) { return tb3_make(n.hx[k], n.hy[k], n.hz[k]); }

/* pq_kernels.hip's walk, one point: nearest child first, the farther one pushed iff its bound does not exceed the culling value of the moment */
NearestBest nearestWalk(const HostScene& s, tb3 p, float limit, std::vector<uint32_t>& stack)
{
    NearestBest best;
    tb3 rc, rh; rootBoxOf(s, rc, rh);
    const float slack = tb_nearest_slack(tb_nearest_scale(p, rc, rh));
    float cull = tb_nearest_cull(limit, slack);
    if (tb_box_d2(p, rc, rh) > cull) return best;
    stack.clear();
    uint32_t ref = s.rootRefB;
    for (;;) {
        if (!(ref & TB_BVH_LEAF_FLAG)) {
            const TbNodeB& n = s.nodesB[ref];
            const float dl = tb_box_d2(p, childCentre(n, 0), childHalf(n, 0)), dr = tb_box_d2(p, childCentre(n, 1), childHalf(n, 1));
            const bool lh = !(dl > cull), rh2 = !(dr > cull);
            if (lh && rh2) { const bool rightFirst = dr < dl; stack.push_back(rightFirst ? n.left : n.right); ref = rightFirst ? n.right : n.left; continue; }
            if (lh || rh2) { ref = rh2 ? n.right : n.left; continue; }
        } else if (nearestOffer(best, p, limit, s.trisB[ref & ~TB_BVH_LEAF_FLAG])) cull = tb_nearest_cull(best.d2, slack);
        if (stack.empty()) return best;
        ref = stack.back(); stack.pop_back();
    }
}

bool nearestSceneOk(const tb_host_scene* h) { return h && h->scene.instances.empty() && !h->scene.trisB.empty() && h->scene.bvhA.size() >= 48; }

} // namespace

int tb_host_scene_nearest(tb_host_scene* h, uint32_t flags, uint64_t n, const TbQueryPoint* points, TbNearest* out)
{
    const uint32_t form = flags & (TB_NEAREST_HOST_BRUTE | TB_NEAREST_HOST_WALK);
    if (!h || (flags & ~(TB_NEAREST_SIGNED | TB_NEAREST_HOST_BRUTE | TB_NEAREST_HOST_WALK)) || (form != TB_NEAREST_HOST_BRUTE && form != TB_NEAREST_HOST_WALK) ||
        (n && (!points || !out))) return TB_E_INVALID;
    if (!h->scene.instances.empty()) return TB_E_UNSUPPORTED;
    if (!nearestSceneOk(h)) return TB_E_INVALID;
    const HostScene& s = h->scene;
    auto range = [&](uint64_t first, uint64_t end) {
        std::vector<uint32_t> stack;
        for (uint64_t i = first; i < end; i++) {
            const tb3 p = cornerOf(points[i].Position);
            const float limit = tb_nearest_limit(points[i].MaxDistance);
            NearestBest best;
            if (tb_nearest_finite3(p) && limit >= 0.0f) {
                if (form == TB_NEAREST_HOST_WALK) best = nearestWalk(s, p, limit, stack);
                else for (const TbTriB& t : s.trisB) nearestOffer(best, p, limit, t);
            }
            out[i] = nearestRecord(best, (flags & TB_NEAREST_SIGNED) != 0);
        }
    };
    /* a point's record depends on nothing but the point: a large brute force is dealt over a few threads */
    const uint64_t work = form == TB_NEAREST_HOST_BRUTE ? n * (uint64_t)s.trisB.size() : n * 64u;
    const uint64_t threads = work < (1ull << 22) ? 1u : std::min<uint64_t>(std::min<uint64_t>(8u, std::max(1u, std::thread::hardware_concurrency())), n);
    std::vector<std::thread> pool;
    uint64_t t = 0;
    try { for (; t + 1 < threads; t++) pool.emplace_back(range, n * t / threads, n * (t + 1) / threads); } catch (const std::exception&) {}
    range(n * t / threads, n); /* the calling thread takes the last share, and what no thread could be started for */
    for (std::thread& th : pool) th.join();
    return TB_OK;
}

int tb_host_scene_nearest_excess(tb_host_scene* h, uint64_t n, const TbQueryPoint* points, float* worstOut)
{
    if (!h || !worstOut || (n && !points)) return TB_E_INVALID;
    if (!h->scene.instances.empty()) return TB_E_UNSUPPORTED;
    if (!nearestSceneOk(h)) return TB_E_INVALID;
    const HostScene& s = h->scene;
    /* per sorted triangle the boxes above it, the root's first: found once, by a walk of the whole tree */
    std::vector<std::vector<std::pair<tb3, tb3>>> above(s.trisB.size());
    {
        tb3 rc, rh; rootBoxOf(s, rc, rh);
        std::vector<std::pair<tb3, tb3>> path(1, std::make_pair(rc, rh));
        std::function<void(uint32_t)> down = [&](uint32_t ref) {
            if (ref & TB_BVH_LEAF_FLAG) { above[ref & ~TB_BVH_LEAF_FLAG] = path; return; }
            const TbNodeB& nd = s.nodesB[ref];
            for (int k = 0; k < 2; k++) { path.push_back(std::make_pair(childCentre(nd, k), childHalf(nd, k))); down(k ? nd.right : nd.left); path.pop_back(); }
        };
        down(s.rootRefB);
    }
    double worst = 0.0;
    for (uint64_t i = 0; i < n; i++) {
        const tb3 p = cornerOf(points[i].Position);
        const float limit = tb_nearest_limit(points[i].MaxDistance);
        if (!tb_nearest_finite3(p) || !(limit >= 0.0f)) continue;
        NearestBest best; size_t winner = 0;
        for (size_t t = 0; t < s.trisB.size(); t++) if (nearestOffer(best, p, limit, s.trisB[t])) winner = t;
        if (best.geom == TB_NEAREST_NONE && best.prim == TB_NEAREST_NONE) continue;
        const double unit = (double)tb_nearest_scale(p, above[winner][0].first, above[winner][0].second) * 1.1920928955078125e-7;
        for (const auto& box : above[winner]) {
            const double excess = sqrt((double)tb_box_d2(p, box.first, box.second)) - sqrt((double)best.d2);
            if (unit > 0.0 && excess / unit > worst) worst = excess / unit;
        }
    }
    *worstOut = (float)worst;
    return TB_OK;
}

/* ---- winding numbers on the host (the rule: include/tb_winding.h; the scalar code: winding_host.h) ------------- */
/* Why tb_winding_numbers (grid null) or tb_bake_winding_field refuses its arguments before it looks at the context: pure tests, in tb_nearest_refusal's
 * order, then beta. */
int tb_winding_refusal(uint32_t flags, uint64_t n, const void* points, const void* out, const tb_probe_grid* grid, float beta, char* why, uint32_t whyBytes)
{
    const char* no = nullptr;
    if (flags & ~(TB_WINDING_DEVICE | (grid ? 0u : TB_WINDING_HOST_WALK))) no = "unknown flag bits";
    else if ((flags & TB_WINDING_DEVICE) && (flags & TB_WINDING_HOST_WALK)) no = "the host walk takes host arrays: flag bits that exclude each other";
    else if (!grid) {
        if (n > (1ull << 31)) no = "more than 2^31 points";
        else if (n && (!points || !out)) no = "null pointer";
        else if (n && (flags & TB_WINDING_DEVICE) && ((uintptr_t)points & 15u)) no = "device points are not 16-B aligned";
        else if (n && (flags & TB_WINDING_DEVICE) && ((uintptr_t)out & 3u)) no = "the device numbers are not 4-B aligned";
    } else no = nearestRefusal(flags & TB_WINDING_DEVICE, 0, nullptr, out, grid, true);
    if (!no && !(beta >= 1.0f)) no = "beta is a NaN or below 1";
    if (why && whyBytes) { strncpy(why, no ? no : "", whyBytes - 1); why[whyBytes - 1] = 0; }
    return no ? TB_E_INVALID : TB_OK;
}

int tb_host_scene_winding(tb_host_scene* h, uint32_t flags, uint64_t n, const TbQueryPoint* points, float beta, float* out)
{
    if (!h || (flags != TB_WINDING_HOST_BRUTE && flags != TB_WINDING_HOST_WALK) || (n && (!points || !out)) || !(beta >= 1.0f)) return TB_E_INVALID;
    if (!h->scene.instances.empty()) return TB_E_UNSUPPORTED;
    if (!nearestSceneOk(h)) return TB_E_INVALID;
    const HostScene& s = h->scene;
    if (s.trisB.size() != s.triGeometry.size()) return TB_E_UNSUPPORTED; /* pre-split references: a sum over the leaves would count a triangle twice */
    const tbwinding::Tree tree{s.nodesB.data(), s.nodesB.size(), s.trisB.data(), s.trisB.size(), s.rootRefB};
    try { tbwinding::run(tree, flags == TB_WINDING_HOST_WALK, n, points, beta, out); } catch (const std::exception&) { return TB_E_INVALID; }
    return TB_OK;
}

} // extern "C"
