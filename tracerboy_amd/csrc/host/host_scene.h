/* host_scene.h -- host-side image of everything the kernels read: the output of the build's
 * restatement of TracerBoy::LoadScene (/root/reference/TracerBoy/TracerBoy.cpp:1065-2161). */
#pragma once
#include "../../../include/tb_abi.h"
#include "../../../include/tracerboy_hip.h"
#include "pbrt_scene.h"

#include <string>
#include <functional>
#include <vector>

namespace tbhost {

struct HostScene {
    tb_camera camera{};
    std::vector<TbMaterial> materials;
    std::vector<TbTextureData> textureData;
    std::vector<TbLight> lights;
    std::vector<TbHitGroupRecord> hitGroups;
    std::vector<float> vertexBuffer;   /* TbVertex, 8 floats per vertex, all meshes back to back */
    std::vector<float> positions;      /* 3 floats per vertex, same vertex numbering             */
    std::vector<uint32_t> indexBuffer; /* mesh-local indices, as the reference uploads them      */
    /* one entry per triangle, in geometry order: what the BVH builder consumes */
    std::vector<uint32_t> triVertexIndex /*3 per tri, absolute into positions*/, triGeometry, triPrimitive, triFlags;
    std::vector<TbImageDesc> images;
    std::vector<TbFloat4> texelPool;
    std::vector<TbFloat4> envMap; uint32_t envWidth = 0, envHeight = 0;
    std::vector<TbFloat4> blueNoise0, blueNoise1;
    TbConfigConstants config{};
    int filmWidth = 0, filmHeight = 0;
    float sceneMin[3] = {0, 0, 0}, sceneMax[3] = {0, 0, 0};
    /* two-level scenes (ConvertOptions::flattenInstances = false): bottom-level structures = triangle ranges of the arrays above
     * (object space, triGeometry = geometry index INSIDE the structure), instances = (structure, transform, first hit-group record) */
    struct Blas { uint32_t firstTri = 0, numTris = 0, offsetA = 0, rootRefB = 0, depth = 0; };
    struct Instance { uint32_t blas = 0; float objectToWorld[12]; float worldToObject[12]; uint32_t hitGroupBase = 0; };
    std::vector<Blas> blas;
    std::vector<Instance> instances;
    std::vector<uint8_t> tlasA;            /* layout A of the top level (tb_abi.h TbBvhMetadata) */
    std::vector<uint32_t> blasOffsets;     /* layout-A image b starts at bvhA[blasOffsets[b]]; numBlas + 1 entries */
    std::vector<TbInstanceB> instancesB;   /* layout B; top-level nodes lead nodesB, a top-level leaf ref is LEAF | instance index */
    /* acceleration structure */
    std::vector<uint8_t> bvhA;
    std::vector<TbNodeB> nodesB;
    std::vector<TbTriB> trisB;
    uint32_t rootRefB = 0;   /* child-ref encoding of the root (leaf bit set when N == 1) */
    uint32_t bvhMaxDepth = 0;
    /* builder 1 (SAH): reinsertion passes after the top-down build; -1 = by size (16 up to 4 096 triangles, 3 above).  Option "reinsertion_passes":
     * on a 700 k-triangle scene the top-down build is ~1 s and every pass ~2.5 s of load time; one pass brings most of what three do
     * (the reference's vw-van at 4K: 62.6 box tests per sample with the GPU-built LBVH + treelets, 58.5 / 54.6 / 54.0 with 0 / 1 / 3 passes) */
    int reinsertionPasses = -1;
    /* ... and how much of the tree a pass takes up again: the largest <share> percent of the subtrees (by surface area), 100 = all.  Option
     * "reinsertion_share".  Measured on the 700 k-triangle van-class scene (SAH cost = sum of the inner nodes' areas, 18 533 after the top-down build):
     * one pass over everything 14 521 in 7.8 s, three 14 330 in 16 s; three passes over the largest 2 % 13 939 in under a second -- moving the small
     * subtrees first costs the large ones their better places. */
    int reinsertionShare = 100;
    /* builder 1: percent of extra references the builder may make by cutting the triangles with the emptiest boxes in two before it builds
     * (bvh_build.cpp presplitReferences; option "presplit"); 0 = one reference per triangle */
    int presplitPercent = 0;
    /* builder 1: the wave stage after the reinsertion passes (bvh_build.cpp optimizeForWaves; option "wave_tree"): -1 = the library's own choice (on where
     * reinsertion passes run), 0 = off, 1 = on.  It runs only for a scene that will be LDS-resident: one level, and within ldsSceneBudget bytes by the size test of lds_image.h
     * (options "lds_scene_budget" / "scene_in_lds"; 0 = no scene is) */
    int waveTree = -1;
    /* ... its workers (option "wave_tree_threads"): 0 = min(16, the CPUs of the process's affinity mask), 1 = serial; the tree is the same bytes for
     * every count.  And the search itself, for comparisons (tb_host_scene_wave_search): the model rays' seed, number of waves and share of feeler
     * waves (0 / 0 / -1 = the stage's own), and how many places per cut subtree are priced: 0 = every legal place, K > 0 = the stage as it was
     * before it priced them all -- the K best by induced area, four passes, no validation rays (K = 3 gives that stage's tree byte for byte) */
    int waveTreeThreads = 0;
    uint32_t waveSearchSeed = 0, waveSearchWaves = 0, waveSearchPlaces = 0, waveSearchKeep = 0 /* finalists of the screen, 0 = the stage's own */; int waveSearchFeelerPercent = -1;
    bool waveSearchVerify = false; /* tests: every place is priced a second time by a plain walk of all rays; a difference throws */
    uint32_t ldsSceneBudget = 40u * 1024u;
    /* what the wave stage did at the last build: costs in wave instructions over its own model rays (wave_cost.h).  evaluations: trees fitted;
     * placesPriced: those inside the depth limit, whose rays were priced; abandoned: of them, stopped early because the partial sum had passed the
     * best price; raysChecked: rays that had visited a changed node and were gone through visit by visit; raysRewalked: of them, walked again from
     * the visit that came out otherwise (all others kept their steps); cutsSkipped: subtrees not cut again in an unchanged tree; validationRejects:
     * winners refused because they raised the price of the validation rays; validation*: that price.  With more
     * than one worker `abandoned` and `raysRewalked` depend on which worker finished first; the tree does not. */
    struct WaveStageReport { uint32_t ran = 0, rays = 0, seed = 0, parkMin = 0, depthLimit = 0, moves = 0, evaluations = 0;
        uint64_t innerBefore = 0, leafBefore = 0, innerAfter = 0, leafAfter = 0; double costBefore = 0, costAfter = 0, milliseconds = 0;
        uint64_t placesPriced = 0, abandoned = 0, raysChecked = 0, raysRewalked = 0; uint32_t threads = 0, passes = 0, places = 0, validationRejects = 0, cutsSkipped = 0;
        uint64_t placesScreened = 0; uint32_t screenWaves = 0, screenKeep = 0; /* the screen: places priced on the first screenWaves waves; screenKeep went on */
        double validationBefore = 0, validationAfter = 0; } waveStage;
};

struct ConvertOptions {
    bool flattenInstances = true; /* reference SW path traces BLAS[0] only and uses shapes[0] of an instance
                                     (TracerBoy.cpp:1370-1375, 2861-2866); the build flattens all of them.  false: the reference's
                                     hardware-path structure -- world-level shapes form one bottom-level structure under an identity
                                     instance, every ObjectInstance becomes an instance of its object's structure (TracerBoy.cpp:1356-1376,
                                     2032-2052), traced by the two-level walk of TraverseFunction.hlsli:603-640 */
    bool flipTextureUVs = true;   /* ConfigConstants.FlipTextureUVs = m_flipTextureUVs: TRUE for .pbrt and .pbf loads ("PBRT uses GL style
                                     texture sampling", TracerBoy.cpp:1207-1208,1221-1222), false only on the Assimp path; option
                                     "flip_texture_uvs" = 0 gives the Assimp convention */
};

/* TracerBoy::LoadScene steps 2-4 (camera :1243-1272, shape loop :1356-1835, lights :1896-1917) */
void ConvertScene(const PbrtScene& in, HostScene& out, const ConvertOptions& opt);

/* BVH build (bvh_build.cpp).  builder 0 = LBVH with the fallback layer's semantics, 1 = binned SAH. */
void BuildBvh(HostScene& scene, int builder);
/* the same with the construction of a single structure / of the top level supplied by the caller (the GPU builders, context.cpp);
 * tlas fills scene.tlasA, the M - 1 layout-B top-level nodes, the root reference and the top level's depth from the structures' root
 * boxes (min xyz, max xyz per structure) */
typedef std::function<void(HostScene&, const std::vector<float>& blasRootBoxes, std::vector<TbNodeB>& topNodes, uint32_t& rootRef,
    uint32_t& depth)> TlasBuilder;
void BuildBvhWith(HostScene& scene, const std::function<void(HostScene&)>& single, const TlasBuilder& tlas);
/* A two-level scene's top level again, from HostScene::instances as they are now (bvh_build.cpp; tb_set_instance_transforms): tlasA, the M - 1
 * top-level nodes at the head of nodesB, instancesB's worldToObject, rootRefB and bvhMaxDepth -- what a build of the scene with those transforms
 * gives.  tlas: as for BuildBvhWith (null: the host's BuildTlas).  The bottom levels are not touched. */
void RebuildTopLevel(HostScene& scene, const TlasBuilder& tlas);
/* the loader's inverse of an instance transform (host_scene.cpp InverseAffineTransform: the fallback layer's fp32 expressions) and its determinant */
void InvertInstanceTransform(const float objectToWorld[12], float worldToObject[12]);
float InstanceTransformDeterminant(const float objectToWorld[12]);
/* builder 1's wave stage (bvh_build.cpp, wave_cost.h): the surfaces its model rays start from, and the size of its ray set */
struct WaveSurfaces;
void WaveSurfacesOf(const HostScene& scene, WaveSurfaces& out);
void WaveStageSize(uint32_t& seed, uint32_t& waves, uint32_t& feelerPercent, uint32_t& places);

/* Procedural stand-ins (procedural.cpp) */
void MakeProceduralScene(HostScene& out, int kind, uint32_t targetTriangles, uint32_t seed);
/* their camera, shared with scenes from arrays: at `eye` looking at `target`, up (0, 1, 0), lens height 2, the focal distance of the field of view */
void SetLookAtCamera(HostScene& s, const float eye[3], const float target[3], float fovDeg);

/* Scenes from caller arrays (host_scene.cpp).  MeshesRefusal: the argument tests of tb_meshes_refusal, empty when there is
 * none.  MeshesToScene: those, then the value checks, then the scene, one geometry per mesh through the functions the PBRT conversion uses; every
 * pointer of desc is host memory.  Returns TB_OK, or the code with the cause in why and `out` untouched.  SmoothNormals: include/tb_normals.h's
 * rule over one mesh; vertices no triangle names are not written. */
std::string MeshesRefusal(const tb_scene_desc* desc);
std::string MeshesUnsupported(const tb_scene_desc& desc); /* a material that names a texture; desc has passed MeshesRefusal */
int MeshesToScene(const tb_scene_desc& desc, HostScene& out, std::string& why);
void SmoothNormals(const float* positions, uint32_t numVertices, const uint32_t* indices, uint32_t numTriangles, float* normalsOut);

/* images (images.cpp): Radiance RGBE .hdr and .pfm -> RGBA32F, top row first; PNG / PFM writers for the output stage */
bool WritePngRGBA8(const std::string& file, uint32_t W, uint32_t H, const uint8_t* rgba, std::string& err);
bool WritePfmRGB(const std::string& file, uint32_t W, uint32_t H, const float* rgba, std::string& err);
bool WriteExrRGBA(const std::string& file, uint32_t W, uint32_t H, const float* rgba, std::string& err);
bool LoadImageRGBA32F(const std::string& file, std::vector<TbFloat4>& texels, uint32_t& w, uint32_t& h, bool& normalizedFormat, std::string& err,
    bool* hasAlpha = nullptr);
/* PNG / TGA (image_decode.cpp): texels as the DXGI typed load of what DirectXTex produces, top row first */
/* D3D12_REQ_TEXTURE2D_U_OR_V_DIMENSION: what the reference could create a texture for; every reader refuses more before it allocates */
inline bool ImageDimensionsOk(uint32_t w, uint32_t h) { return w >= 1 && h >= 1 && w <= 16384 && h <= 16384; }
struct DecodedImage { std::vector<TbFloat4> texels; uint32_t width = 0, height = 0; bool normalized = false, hasAlpha = false; };
bool DecodeImageFile(const std::string& file, DecodedImage& img, std::string& err);

/* the two 256x256 RGBA8 blue-noise tiles (t14/t15) from tracerboy_amd/data; false when absent */
bool LoadBlueNoiseTiles(HostScene& scene);

void DefaultOutputSettings(tb_output_settings& s);
/* TracerBoy.cpp:2808-2851 */
void MakeFrameConstants(const HostScene& scene, const tb_camera& cam, const tb_output_settings& s, uint32_t frame, float timeSeed,
                        uint32_t selX, uint32_t selY, TbPerFrameConstants& out);

} // namespace tbhost
