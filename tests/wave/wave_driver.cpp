/* wave_driver.cpp -- wave_cost.h and builder 1's wave stage (tracerboy_amd/csrc/host/bvh_build.cpp) as a host program with its own main, built with
 * ASan + UBSan (tests/wave/Makefile; tests/test_wave_cost.py reads what it prints).  The scene is made by hand: a closed room of 12 triangles, two
 * blocks of 12 and a light of 2 under the ceiling, 38 triangles, small enough to be LDS-resident.  Prints
 *   replay_<case> inner leaf idle       hand-written step strings
 *   stage ran <cost before> <cost after> <moves>
 *   walk_matches_brute_force 0|1        the closest t of the walk over the built tree against every triangle tested in turn */
#include <cstdio>
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

static bool treeOf(const HostScene& s, WaveTree& w)
{
    uint32_t hdr[4]; memcpy(hdr, s.bvhA.data(), 16);
    const uint32_t N = (uint32_t)s.trisB.size();
    const TbAabbNode* nodes = (const TbAabbNode*)(s.bvhA.data() + hdr[0]);
    w.N = N; w.center.resize(2 * N - 1); w.half.resize(2 * N - 1); w.left.assign(N - 1, 0); w.right.assign(N - 1, 0); w.v0.resize(N); w.v1.resize(N); w.v2.resize(N);
    for (uint32_t i = 0; i < 2 * N - 1; i++) {
        w.center[i] = tb3_make(nodes[i].center[0], nodes[i].center[1], nodes[i].center[2]); w.half[i] = tb3_make(nodes[i].halfDim[0], nodes[i].halfDim[1], nodes[i].halfDim[2]);
        if (i < N - 1) { w.left[i] = nodes[i].flags & TB_BVH_INDEX_MASK; w.right[i] = nodes[i].rightNodeIndex; if (w.left[i] >= 2 * N - 1 || w.right[i] >= 2 * N - 1) return false; }
    }
    for (uint32_t k = 0; k < N; k++) { w.v0[k] = tb3_make(s.trisB[k].v0[0], s.trisB[k].v0[1], s.trisB[k].v0[2]); w.v1[k] = tb3_make(s.trisB[k].v1[0], s.trisB[k].v1[1], s.trisB[k].v1[2]);
        w.v2[k] = tb3_make(s.trisB[k].v2[0], s.trisB[k].v2[1], s.trisB[k].v2[2]); }
    return true;
}

static void replay(const char* name, std::vector<const char*> steps, uint32_t parkMin)
{
    std::vector<uint32_t> len; for (const char* s : steps) len.push_back((uint32_t)strlen(s));
    const WaveTrips w = WaveReplay(steps.data(), len.data(), (uint32_t)steps.size(), parkMin);
    printf("%s %llu %llu %llu\n", name, (unsigned long long)w.inner, (unsigned long long)w.leaf, (unsigned long long)w.idle);
}

int main()
{
    replay("replay_one_lane", {"IIL"}, 2);
    replay("replay_threshold", {"IIIL", "IIIL", "IL"}, 3);
    replay("replay_idle", {"", ""}, 2);
    { std::vector<const char*> full(64, "IILIL"); replay("replay_full_wave", full, 2); }

    HostScene s;
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
    s.waveTree = 1;
    BuildBvh(s, 1);
    const HostScene::WaveStageReport& r = s.waveStage;
    printf("stage %s %.0f %.0f %u\n", r.ran ? "ran" : "skipped", r.costBefore, r.costAfter, r.moves);

    WaveTree w; if (!treeOf(s, w)) { printf("walk_matches_brute_force 0\n"); return 1; }
    WaveSurfaces surf; WaveSurfacesOf(s, surf);
    std::vector<WaveRay> rays; WaveModelRays(surf, 7u, 16, 40, rays);
    /* ... and rays with a zero component and a NaN, which take the degenerate-axis constants and the miss-at-once rule */
    { WaveRay a; a.o = tb3_make(0, 1, 0); a.d = tb3_make(0, 0, 1); a.tMax = kWaveMaxT; WaveRayPrepare(a); rays.push_back(a);
      WaveRay b = a; b.d = tb3_make(0, -1, 0); WaveRayPrepare(b); rays.push_back(b);
      WaveRay c = a; c.o.x = std::nanf(""); WaveRayPrepare(c); rays.push_back(c); }
    bool same = true; std::vector<char> steps;
    for (const WaveRay& ray : rays) {
        steps.clear();
        const float walked = WaveWalk(w, ray, steps);
        float brute = ray.tMax;
        if (!ray.cannotHit) for (uint32_t k = 0; k < w.N; k++) { float t0 = brute; WaveTriTest(t0, ray, w.v0[k], w.v1[k], w.v2[k]); if (t0 < brute && t0 > kWaveMinT) brute = t0; }
        if (walked != brute) same = false;
    }
    std::vector<char> arena;
    const WaveTrips total = WaveCostOfTree(w, rays, 2, arena);
    printf("walk_matches_brute_force %d\n", same ? 1 : 0);
    printf("trips %llu %llu %llu\n", (unsigned long long)total.inner, (unsigned long long)total.leaf, (unsigned long long)total.idle);
    return 0;
}
