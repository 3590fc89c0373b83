/* lds_image.h -- the LDS image of the walk (kernels/pt_scene.h TbDeviceScene::ldsBlob), built by a pure host function: no context, no device.
 * context_scene.cpp uploads what it returns; tb_host_scene_lds_image (host_api.cpp) hands it to the CPU tests, which walk it. */
#pragma once
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>
#include "../kernels/pt_scene.h"

struct LdsImage { std::vector<uint8_t> bytes; uint32_t offNodes = 0, offTris = 0; };

inline size_t LdsImageBytes(size_t numNodes, size_t numTris)
{
    return (numNodes * TB_LDS_NODE_STRIDE + 15) / 16 * 16 + (numTris * TB_LDS_TRI_COPIES * sizeof(TbTriB) + 15) / 16 * 16;
}

/* parkMin of a scene in LDS where option "park_min" is not set (context_scene.cpp has the measurements; the wave stage replays with it) */
constexpr uint32_t kLdsSceneParkMin = 2;

/* What the budget of an LDS-resident scene counts (option "lds_scene_budget"), from the counts alone: the image, the shading records in their device
 * form -- they stay in memory (pt_scene.h), the budget still counts them, so that which scenes are LDS-resident is as it was -- and the stacks of a
 * workgroup.  context_scene.cpp decides with it, and builder 1 asks it before the scene is built (bvh_build.cpp, the wave stage). */
inline size_t LdsSceneBytes(size_t numNodes, size_t numTris, size_t numHitGroups, size_t numIndices, size_t numVertexFloats, size_t numMaterials,
    size_t numLights, uint32_t stackDepth)
{
    auto r16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t shadingBytes = r16(numHitGroups * sizeof(TbDevHitGroup)) + r16(numIndices * 4) + r16(numVertexFloats * 4) +
        r16(numMaterials * sizeof(TbDevMaterial)) + r16(numLights * sizeof(TbDevLight));
    return LdsImageBytes(numNodes, numTris) + shadingBytes + (size_t)stackDepth * 256 * 4;
}

/* Nodes first, TB_LDS_NODE_STRIDE apart, then TB_LDS_TRI_COPIES axis-permuted copies of every triangle (copy = kz * 2 + swapped, (kx, ky) = the
 * two axes after kz, swapped when d[kz] < 0).  Child refs are offsets in 16-B units (pt_scene.h): an inner ref from the first node record, a leaf
 * ref -- leaf flag in the sign bit -- from the first triangle record to the triangle's first copy.  The root's ref, 0 or LEAF | 0, is the same
 * as in every image.  (The kernels that walk with the LDS steps turn the refs of their own copy into addresses on the way in: pt_device.hpp.) */
inline LdsImage BuildLdsImage(const TbNodeB* nodes, size_t numNodes, const TbTriB* tris, size_t numTris)
{
    if (LdsImageBytes(numNodes, numTris) > 0x7fffffffull)
        throw std::runtime_error("scene too large for an LDS image");
    LdsImage im;
    auto ldsRef = [](uint32_t ref) { return (ref & TB_BVH_LEAF_FLAG) ? (TB_BVH_LEAF_FLAG | ((ref & ~TB_BVH_LEAF_FLAG) * ((uint32_t)sizeof(TbTriB) / 16u) * TB_LDS_TRI_COPIES)) :
        ref * (TB_LDS_NODE_STRIDE / 16u); };
    im.offNodes = 0;
    im.bytes.assign(numNodes * TB_LDS_NODE_STRIDE, 0);
    for (size_t i = 0; i < numNodes; i++) {
        TbNodeB nd = nodes[i]; nd.left = ldsRef(nd.left); nd.right = ldsRef(nd.right);
        memcpy(im.bytes.data() + i * TB_LDS_NODE_STRIDE, &nd, sizeof nd);
    }
    while (im.bytes.size() % 16) im.bytes.push_back(0);
    im.offTris = (uint32_t)im.bytes.size();
    im.bytes.resize(im.offTris + numTris * TB_LDS_TRI_COPIES * sizeof(TbTriB));
    for (size_t i = 0; i < numTris; i++)
        for (int kz = 0; kz < 3; kz++)
            for (int sw = 0; sw < 2; sw++) {
                int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
                if (sw) std::swap(kx, ky);
                const TbTriB& t = tris[i]; TbTriB q = t;
                const float* src[3] = {t.v0, t.v1, t.v2}; float* dst[3] = {q.v0, q.v1, q.v2};
                for (int v = 0; v < 3; v++) { dst[v][0] = src[v][kx]; dst[v][1] = src[v][ky]; dst[v][2] = src[v][kz]; }
                memcpy(im.bytes.data() + im.offTris + (i * TB_LDS_TRI_COPIES + (size_t)(kz * 2 + sw)) * sizeof(TbTriB), &q, sizeof q);
            }
    while (im.bytes.size() % 16) im.bytes.push_back(0);
    return im;
}

/* Whether every index the kernels can form into the shading tables is in range (pt_device.hpp fetch_surface, load_vertex, fetch_material,
 * shadow_hit_is_light): for every triangle record its geometry index, the index triple of its primitive, the three vertices the triple names and
 * the hit group's material.  The tables in their device form: hit groups with offsets in elements, vertices as floats, 8 per vertex.  Sums in 64
 * bits: an index near 2^32, whose 32-bit sum would wrap into range on the device, is out of range here.  The copy whose fetches carry no bounds
 * check (kernels/pt_variant_matte6.hip) runs only for a scene this holds for (context_render.cpp pickCopy); light indices are checked per call. */
inline bool SceneTablesInRange(const TbTriB* tris, size_t numTris, const TbDevHitGroup* hitGroups, size_t numHitGroups, const uint32_t* indices,
    size_t numIndices, size_t numVertexFloats, size_t numMaterials)
{
    for (size_t i = 0; i < numTris; i++) {
        if (tris[i].geometryIndex >= numHitGroups) return false;
        const TbDevHitGroup& g = hitGroups[tris[i].geometryIndex];
        const uint64_t iAt = (uint64_t)g.iFirst + 3ull * tris[i].primitiveIndex;
        if (iAt + 3ull > numIndices) return false;
        for (int k = 0; k < 3; k++)
            if (8ull * indices[iAt + k] + g.vFirst + 8ull > numVertexFloats) return false;
        if (g.MaterialIndex >= numMaterials) return false;
    }
    return true;
}

/* entries per lane of the traversal stack: a root-to-leaf path of bvhMaxDepth nodes has bvhMaxDepth - 1 inner nodes, each of which parks at most
 * one far child, so a walk never holds more than bvhMaxDepth - 1 entries.  The spare one is entry 0 of the walks that keep a sentinel there
 * (pt_device.hpp, the LDS steps) */
inline uint32_t WalkStackDepth(uint32_t bvhMaxDepth) { return bvhMaxDepth < 2 ? 2 : bvhMaxDepth; }
