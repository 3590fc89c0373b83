/* search_driver.cpp -- the search of builder 1's wave stage (tracerboy_amd/csrc/host/bvh_build.cpp optimizeForWaves, docs/experiments/r13.md) as a host
 * program with its own main, built once with ASan + UBSan and once with TSan (tests/wave_search/Makefile; tests/test_wave_search.py reads what it
 * prints).  The scene is the hand-made room of tests/wave/wave_driver.cpp: 12 triangles of walls, two blocks of 12, a light of 2 -- 38 triangles, small
 * enough to be LDS-resident.
 *   search_driver [threads [verify|plain [waves]]]     (default 4 workers, no verification, the stage's own 24 waves)
 * builds its tree three times: the three best places by area (the stage as it was), every place with one worker, every place with `threads` workers.
 * Prints
 *   by_area  <cost before> <cost after> <moves> <places priced>
 *   serial   <cost before> <cost after> <moves> <places priced> <abandoned> <rays rewalked> <passes> <validation before> <validation after> <rejects>
 *   threaded <the same> <workers>
 *   same_tree 0|1               the serial and the threaded search gave the same layout-A bytes
 *   priced_right 0|1            the stage's price of its tree is the price of a plain walk of its rays over the image that was built
 * and returns 0 when both are 1 and neither the search's own rays nor the validation rays price the full search's tree above the tree it started from. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "host_scene.h"
#include "wave_cost.h"

using namespace tbhost;

bool tbhost::LoadBlueNoiseTiles(HostScene&) { return false; } /* the build binds the system textures with the scene; this program renders nothing */

static void quad(HostScene& s, uint32_t geom, tb3 a, tb3 b, tb3 c, tb3 d)
{
    const uint32_t base = (uint32_t)(s.positions.size() / 3);
    for (const tb3& p : {a, b, c, d}) { s.positions.push_back(p.x); s.positions.push_back(p.y); s.positions.push_back(p.z); }
    const uint32_t idx[6] = {0, 1, 2, 0, 2, 3};
    for (int t = 0; t < 2; t++) {
        for (int k = 0; k < 3; k++) s.triVertexIndex.push_back(base + idx[3 * t + k]);
        s.triGeometry.push_back(geom); s.triPrimitive.push_back((uint32_t)s.triPrimitive.size()); s.triFlags.push_back(1);
    }
}
static void box(HostScene& s, uint32_t geom, tb3 lo, tb3 hi)
{
    const tb3 p[8] = {tb3_make(lo.x, lo.y, lo.z), tb3_make(hi.x, lo.y, lo.z), tb3_make(hi.x, hi.y, lo.z), tb3_make(lo.x, hi.y, lo.z),
                      tb3_make(lo.x, lo.y, hi.z), tb3_make(hi.x, lo.y, hi.z), tb3_make(hi.x, hi.y, hi.z), tb3_make(lo.x, hi.y, hi.z)};
    quad(s, geom, p[0], p[1], p[2], p[3]); quad(s, geom, p[4], p[5], p[6], p[7]); quad(s, geom, p[0], p[1], p[5], p[4]);
    quad(s, geom, p[3], p[2], p[6], p[7]); quad(s, geom, p[0], p[3], p[7], p[4]); quad(s, geom, p[1], p[2], p[6], p[5]);
}

static void room(HostScene& s)
{
    TbMaterial matte; memset(&matte, 0, sizeof matte); matte.Flags = TB_MAT_DEFAULT;
    TbMaterial lamp = matte; lamp.Flags = TB_MAT_LIGHT;
    s.materials = {matte, lamp};
    TbHitGroupRecord g; memset(&g, 0, sizeof g); s.hitGroups.push_back(g); g.MaterialIndex = 1; s.hitGroups.push_back(g);
    box(s, 0, tb3_make(-1, 0, -1), tb3_make(1, 2, 1));
    box(s, 0, tb3_make(-0.7f, 0, -0.6f), tb3_make(-0.2f, 1.2f, -0.1f));
    box(s, 0, tb3_make(0.2f, 0, 0.1f), tb3_make(0.7f, 0.6f, 0.6f));
    quad(s, 1, tb3_make(-0.25f, 1.98f, -0.25f), tb3_make(0.25f, 1.98f, -0.25f), tb3_make(0.25f, 1.98f, 0.25f), tb3_make(-0.25f, 1.98f, 0.25f));
    for (int t = 0; t < 2; t++) { /* the light's two triangles */
        TbLight l; memset(&l, 0, sizeof l); l.LightType = TB_LIGHT_TYPE_AREA; l.SurfaceArea = 0.125f;
        const uint32_t* vi = &s.triVertexIndex[3 * (s.triGeometry.size() - 2 + t)];
        const float* p0 = &s.positions[3 * vi[0]], *p1 = &s.positions[3 * vi[1]], *p2 = &s.positions[3 * vi[2]];
        l.P0 = TbFloat3{p0[0], p0[1], p0[2]}; l.P1 = TbFloat3{p1[0], p1[1], p1[2]}; l.P2 = TbFloat3{p2[0], p2[1], p2[2]};
        s.lights.push_back(l);
    }
}

/* the stage's own rays walked one by one over the image that was built */
static double plainPrice(const HostScene& s)
{
    uint32_t hdr[4]; memcpy(hdr, s.bvhA.data(), 16);
    const uint32_t N = (uint32_t)s.trisB.size();
    const TbAabbNode* nodes = (const TbAabbNode*)(s.bvhA.data() + hdr[0]);
    WaveTree w; w.N = N; w.center.resize(2 * N - 1); w.half.resize(2 * N - 1); w.left.assign(N - 1, 0); w.right.assign(N - 1, 0); w.v0.resize(N); w.v1.resize(N);
    w.v2.resize(N);
    for (uint32_t i = 0; i < 2 * N - 1; i++) {
        w.center[i] = tb3_make(nodes[i].center[0], nodes[i].center[1], nodes[i].center[2]); w.half[i] = tb3_make(nodes[i].halfDim[0], nodes[i].halfDim[1], nodes[i].halfDim[2]);
        if (i < N - 1) { w.left[i] = nodes[i].flags & TB_BVH_INDEX_MASK; w.right[i] = nodes[i].rightNodeIndex; }
    }
    for (uint32_t k = 0; k < N; k++) { w.v0[k] = tb3_make(s.trisB[k].v0[0], s.trisB[k].v0[1], s.trisB[k].v0[2]); w.v1[k] = tb3_make(s.trisB[k].v1[0], s.trisB[k].v1[1], s.trisB[k].v1[2]);
        w.v2[k] = tb3_make(s.trisB[k].v2[0], s.trisB[k].v2[1], s.trisB[k].v2[2]); }
    uint32_t seed, waves, feelers, places; WaveStageSize(seed, waves, feelers, places);
    WaveSurfaces surf; WaveSurfacesOf(s, surf);
    std::vector<WaveRay> rays; WaveModelRays(surf, s.waveStage.seed, s.waveStage.rays / kWaveLanes, feelers, rays);
    std::vector<char> arena;
    return WaveCostOfTree(w, rays, s.waveStage.parkMin, arena).cost();
}

static uint32_t g_waves = 0;  /* waves of model rays, 0 = the stage's own 24 (the sanitizer runs take fewer: they are many times slower) */
static bool g_verify = false; /* every place priced a second time by a plain walk of all rays (HostScene::waveSearchVerify): a difference throws */

static HostScene search(const char* name, uint32_t places, int threads)
{
    HostScene s; room(s);
    s.waveTree = 1; s.waveSearchPlaces = places; s.waveTreeThreads = threads; s.waveSearchVerify = g_verify; s.waveSearchWaves = g_waves;
    BuildBvh(s, 1);
    const HostScene::WaveStageReport& r = s.waveStage;
    if (places) printf("%s %.0f %.0f %u %llu\n", name, r.costBefore, r.costAfter, r.moves, (unsigned long long)r.placesPriced);
    else printf("%s %.0f %.0f %u %llu %llu %llu %u %.0f %.0f %u %u\n", name, r.costBefore, r.costAfter, r.moves, (unsigned long long)r.placesPriced,
        (unsigned long long)r.abandoned, (unsigned long long)r.raysRewalked, r.passes, r.validationBefore, r.validationAfter, r.validationRejects, r.threads);
    return s;
}

int main(int argc, char** argv)
{
    const int threads = argc > 1 ? atoi(argv[1]) : 4;
    g_verify = argc > 2 && !strcmp(argv[2], "verify");
    g_waves = argc > 3 ? (uint32_t)atoi(argv[3]) : 0;
    const HostScene byArea = search("by_area", 3, 1), serial = search("serial", 0, 1), threaded = search("threaded", 0, threads);
    const bool same = serial.bvhA == threaded.bvhA && serial.waveStage.costAfter == threaded.waveStage.costAfter;
    const bool right = plainPrice(serial) == serial.waveStage.costAfter && plainPrice(byArea) == byArea.waveStage.costAfter;
    printf("same_tree %d\n", same ? 1 : 0);
    printf("priced_right %d\n", right ? 1 : 0);
    return same && right && serial.waveStage.ran && serial.waveStage.costAfter <= serial.waveStage.costBefore &&
        serial.waveStage.validationAfter <= serial.waveStage.validationBefore ? 0 : 1;
}
