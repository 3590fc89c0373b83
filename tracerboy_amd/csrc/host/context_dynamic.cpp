/* context_dynamic.cpp -- dynamic scenes (include/tracerboy_hip.h tb_update_positions .. tb_commit_geometry): vertices and instance
 * transforms staged by the caller, applied by a commit.  Moved vertices are refit into the tree as it stands (kernels/refit_kernels.hip: the topology,
 * and so the schedule of the bottom-up pass, is known beforehand); instance transforms rebuild the small top level.  The host copies of the geometry go
 * stale at a commit and are brought up on first demand (refreshHostScene). */
#include "query_call.h"
#include "lds_image.h"
#include "tb_vec.h"
#include "../kernels/refit_launch.h"

#include <cstdlib>

using namespace tbhost;
using namespace tbctx;

/* The slots and the schedule of a bottom-up pass over the host's tree, whose child refs never go stale (refit_launch.h RefitTables: triSlot, nodeSlot,
 * schedule; levelFirst: the nodes of height h are schedule[levelFirst[h - 1] .. levelFirst[h])).  The refit's tables and the winding numbers' moment
 * fit (context_winding.cpp) are both made of it. */
void tbctx::treeSchedule(const HostScene& s, std::vector<uint32_t>& triSlot, std::vector<uint32_t>& nodeSlot, std::vector<uint32_t>& schedule,
    std::vector<uint32_t>& levelFirst)
{
    const size_t N = s.trisB.size(), numNodes = s.nodesB.size();
    triSlot.assign(N, REFIT_ROOT_SLOT); nodeSlot.assign(numNodes, REFIT_ROOT_SLOT); schedule.clear();
    std::vector<uint32_t> height(numNodes, 0);
    levelFirst.assign(1, 0u);
    if (!(s.rootRefB & TB_BVH_LEAF_FLAG)) {
        std::vector<uint32_t> walk; walk.reserve(numNodes);
        std::vector<uint32_t> st(1, s.rootRefB);
        if (s.rootRefB >= numNodes) throw std::runtime_error("dynamic geometry: the root is out of range");
        while (!st.empty()) {
            const uint32_t x = st.back(); st.pop_back(); walk.push_back(x);
            if (walk.size() > numNodes) throw std::runtime_error("dynamic geometry: the tree is not a tree");
            const uint32_t child[2] = {s.nodesB[x].left, s.nodesB[x].right};
            for (uint32_t side = 0; side < 2; side++) {
                const uint32_t r = child[side], i = r & ~TB_BVH_LEAF_FLAG;
                if (r & TB_BVH_LEAF_FLAG) { if (i >= N) throw std::runtime_error("dynamic geometry: a leaf is out of range"); triSlot[i] = x * 2 + side; }
                else { if (i >= numNodes) throw std::runtime_error("dynamic geometry: a node is out of range"); nodeSlot[i] = x * 2 + side; st.push_back(i); }
            }
        }
        uint32_t maxHeight = 0;
        for (size_t w = walk.size(); w-- > 0;) { /* children come after their parent in a pre-order walk */
            const uint32_t x = walk[w]; uint32_t h = 0;
            for (uint32_t r : {s.nodesB[x].left, s.nodesB[x].right}) if (!(r & TB_BVH_LEAF_FLAG)) h = std::max(h, height[r]);
            height[x] = h + 1; maxHeight = std::max(maxHeight, h + 1);
        }
        std::vector<uint32_t> count(maxHeight + 1, 0u);
        for (uint32_t x : walk) count[height[x]]++;
        levelFirst.assign(maxHeight + 1, 0u); /* the nodes of height h: schedule[levelFirst[h - 1] .. levelFirst[h]) */
        for (uint32_t h = 1; h <= maxHeight; h++) levelFirst[h] = levelFirst[h - 1] + count[h];
        schedule.resize(walk.size());
        std::vector<uint32_t> fill(levelFirst.begin(), levelFirst.end() - 1);
        for (uint32_t x : walk) schedule[fill[height[x] - 1]++] = x;
    }
}

namespace {

typedef tb_context::Dynamic Dynamic;
typedef std::vector<std::pair<uint32_t, uint32_t>> Ranges; /* [first, end) */

uint32_t numVertices(const tb_context* c) { return (uint32_t)(c->scene.positions.size() / 3); }
bool twoLevel(const tb_context* c) { return !c->scene.instances.empty(); }

Dynamic& dynamicOf(tb_context* c) { if (!c->dyn) c->dyn.reset(new Dynamic()); return *c->dyn; }

/* The tables of a refit (refit_launch.h), from the host's tree, which is fresh whenever they are made: the dynamic state is made before the first
 * commit and dropped by a rebuild. */
void makeTables(tb_context* c, Dynamic& d)
{
    const HostScene& s = c->scene;
    const size_t N = s.trisB.size(), numNodes = s.nodesB.size();
    if (N != s.triGeometry.size()) throw std::runtime_error("unsupported: the tree holds pre-split references (option presplit), which a refit cannot fit");
    /* sorted triangle k -> input triangle, by (geometry, primitive) */
    std::vector<std::pair<uint64_t, uint32_t>> byKey(N);
    for (size_t i = 0; i < N; i++) byKey[i] = {((uint64_t)s.triGeometry[i] << 32) | s.triPrimitive[i], (uint32_t)i};
    std::sort(byKey.begin(), byKey.end());
    d.hostTriVerts.resize(3 * N);
    for (size_t k = 0; k < N; k++) {
        const uint64_t key = ((uint64_t)s.trisB[k].geometryIndex << 32) | s.trisB[k].primitiveIndex;
        auto it = std::lower_bound(byKey.begin(), byKey.end(), std::make_pair(key, 0u));
        if (it == byKey.end() || it->first != key) throw std::runtime_error("dynamic geometry: a triangle of the tree is not one of the scene's");
        for (int j = 0; j < 3; j++) {
            const uint32_t v = s.triVertexIndex[3ull * it->second + j];
            if (v >= numVertices(c)) throw std::runtime_error("dynamic geometry: a vertex index is out of range");
            d.hostTriVerts[3 * k + j] = v;
        }
    }
    std::vector<uint32_t> triSlot, nodeSlot, schedule;
    treeSchedule(s, triSlot, nodeSlot, schedule, d.levelFirst);
    uploadInto(c, d.triVerts, d.hostTriVerts); uploadInto(c, d.triSlot, triSlot); uploadInto(c, d.nodeSlot, nodeSlot); uploadInto(c, d.schedule, schedule);
    uploadInto(c, d.positions, s.positions); uploadInto(c, d.levelFirstDevice, d.levelFirst);
    ensure(d.rootBox, 32);
    HIP_TRY(hipStreamSynchronize(c->stream)); /* the vectors above go out of scope */
    d.ready = true;
}

/* The tables of a normal recomputation (refit_launch.h RefitNormalTables), from the scene's per-triangle arrays, which no commit changes: the
 * triangles' vertex numbers in geometry order, and per vertex the face-vector slots of the corners that name it -- triangles ascending, corners
 * 0, 1, 2, which inside one mesh is ascending primitive index: include/tb_normals.h's order.  Emissive geometries' vertices get an empty row. */
void makeNormalTables(tb_context* c, Dynamic& d)
{
    const HostScene& s = c->scene;
    const size_t N = s.triGeometry.size(), V = numVertices(c);
    auto emissive = [&](size_t t) {
        const uint32_t g = s.triGeometry[t];
        if (g >= s.hitGroups.size()) return true; /* no such geometry: not walked */
        const uint32_t m = s.hitGroups[g].MaterialIndex;
        return m < s.materials.size() && (s.materials[m].Flags & TB_MAT_LIGHT) != 0;
    };
    std::vector<uint32_t> rowStart(V + 1, 0u);
    for (size_t t = 0; t < N; t++) for (int k = 0; k < 3; k++) {
        const uint32_t v = s.triVertexIndex[3 * t + k];
        if (v >= V) throw std::runtime_error("dynamic geometry: a vertex index is out of range");
        if (!emissive(t)) rowStart[v + 1]++;
    }
    for (size_t v = 0; v < V; v++) {
        if ((uint64_t)rowStart[v] + rowStart[v + 1] > 0xffffffffull) throw std::runtime_error("dynamic geometry: too many corners");
        rowStart[v + 1] += rowStart[v];
    }
    std::vector<uint32_t> slots(rowStart[V]), fill(rowStart.begin(), rowStart.end() - 1);
    for (size_t t = 0; t < N; t++) if (!emissive(t)) for (int k = 0; k < 3; k++) slots[fill[s.triVertexIndex[3 * t + k]]++] = (uint32_t)t;
    d.normalSlots = rowStart[V];
    uploadInto(c, d.normalTriVerts, s.triVertexIndex); uploadInto(c, d.normalRowStart, rowStart); uploadInto(c, d.normalSlotTable, slots);
    ensure(d.faceVectors, std::max<size_t>(16, 12ull * N));
    HIP_TRY(hipStreamSynchronize(c->stream)); /* the vectors above go out of scope */
    d.normalTablesReady = true;
}

/* the normals of the marked ranges again, chained on the stream after the refit's launches and the explicit normals */
void recomputeNormals(tb_context* c, Dynamic& d, bool afterRefit)
{
    RefitNormalTables t{};
    t.positions = (const float*)d.positions.p; t.triVerts = (const uint32_t*)d.normalTriVerts.p; t.rowStart = (const uint32_t*)d.normalRowStart.p;
    t.slots = (const uint32_t*)d.normalSlotTable.p; t.faceVectors = (float*)d.faceVectors.p; t.vertexBuffer = (float*)c->ds.vertexBuffer;
    t.numTris = (uint32_t)c->scene.triGeometry.size(); t.numVertices = numVertices(c); t.numSlots = d.normalSlots;
    HIP_TRY(hipEventRecord(d.evNormals[0].create(), c->stream));
    HIP_TRY(refit_launch_face_vectors(c->stream, &t));
    for (const auto& r : d.markedNormals) HIP_TRY(refit_launch_vertex_normals(c->stream, &t, r.first, r.second - r.first));
    HIP_TRY(hipEventRecord(d.evNormals[1].create(), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, d.evNormals[0], d.evNormals[1]));
    d.lastMs = (afterRefit ? d.lastMs : 0.0f) + ms;
}

void addRange(Ranges& r, uint32_t first, uint32_t n) { if (n) r.emplace_back(first, first + n); }
void mergeRanges(Ranges& r)
{
    std::sort(r.begin(), r.end());
    Ranges out;
    for (const auto& x : r) { if (!out.empty() && x.first <= out.back().second) out.back().second = std::max(out.back().second, x.second); else out.push_back(x); }
    r.swap(out);
}

/* the vertex range of hit-group record g: its vertices lie from its offset to the next larger offset of any record */
void vertexRangeOf(const HostScene& s, uint32_t g, uint32_t& first, uint32_t& count)
{
    const uint32_t off = s.hitGroups[g].VertexBufferOffset;
    uint32_t next = (uint32_t)(s.vertexBuffer.size() * 4);
    for (const TbHitGroupRecord& h : s.hitGroups) if (h.VertexBufferOffset > off) next = std::min(next, h.VertexBufferOffset);
    first = off / 32; count = (next - off) / 32;
}

/* Staged vertices of an emissive geometry that differ from what the scene holds: the geometry's index, or -1.  Its lights carry the positions and
 * normals (host_scene.cpp AppendAreaLights) and are not made again, so its vertices have never moved and the host copies of them are never stale. */
int movedEmissiveGeometry(tb_context* c, const Ranges& dirty, const DevBuf& staged, bool normals)
{
    const HostScene& s = c->scene;
    if (dirty.empty()) return -1;
    std::vector<float> got, have;
    for (uint32_t g = 0; g < (uint32_t)s.hitGroups.size(); g++) {
        const uint32_t m = s.hitGroups[g].MaterialIndex;
        if (m >= s.materials.size() || !(s.materials[m].Flags & TB_MAT_LIGHT)) continue;
        uint32_t first, count; vertexRangeOf(s, g, first, count);
        for (const auto& r : dirty) {
            const uint32_t lo = std::max(first, r.first), hi = std::min(first + count, r.second);
            if (lo >= hi) continue;
            got.resize(3ull * (hi - lo)); have.resize(got.size());
            HIP_TRY(hipMemcpy(got.data(), (const float*)staged.p + 3ull * lo, got.size() * 4, hipMemcpyDeviceToHost));
            for (uint32_t v = lo; v < hi; v++) for (int k = 0; k < 3; k++)
                have[3ull * (v - lo) + k] = normals ? s.vertexBuffer[8ull * v + k] : s.positions[3ull * v + k];
            if (memcmp(got.data(), have.data(), got.size() * 4) != 0) return (int)g;
        }
    }
    return -1;
}

void dropCompactNodes(tb_context* c)
{
    if (c->ds.nodesC)
        for (size_t i = 0; i < c->sceneBufs.size(); i++) if (c->sceneBufs[i].p == (const void*)c->ds.nodesC) { c->sceneBufs.erase(c->sceneBufs.begin() + i); break; }
    c->ds.nodesC = nullptr; c->compactTried = false;
}

/* what every commit that changed something leaves behind (finalizeScene's own resets) */
void sceneChanged(tb_context* c) { c->sceneGeneration++; resetHistory(c); }

const char* updateRefusal(tb_context* c, const char* what, uint32_t flags, uint32_t first, uint32_t n, const float* xyz, int& code)
{
    code = TB_E_INVALID;
    if (!c->hasScene) { code = TB_E_NO_SCENE; return "no scene loaded"; }
    if (twoLevel(c)) { code = TB_E_UNSUPPORTED; return "vertex updates inside a two-level scene (option flatten_instances = 0 with instances) are not supported"; }
    if (flags & ~TB_UPDATE_DEVICE) return "unknown flag bits";
    if ((uint64_t)first + n > numVertices(c)) return "the vertex range runs past the scene's vertices";
    if (n && !xyz) return "null pointer";
    return nullptr;
}

int stageVertices(tb_context* c, const char* what, bool normals, uint32_t flags, uint32_t first, uint32_t n, const float* xyz)
{
    TB_REFUSE_PEER(c);
    if (c && !c->group.peers.empty()) return fail(c, TB_E_UNSUPPORTED, std::string(what) + ": not supported for a multi-device group");
    return guarded(c, [&]() {
        int code;
        if (const char* why = updateRefusal(c, what, flags, first, n, xyz, code)) return fail(c, code, std::string(what) + ": " + why);
        if (n == 0) return TB_OK;
        const size_t bytes = 12ull * n;
        const bool device = (flags & TB_UPDATE_DEVICE) != 0;
        if (device) checkDevicePointer(c, what, "xyz", xyz, bytes);
        else for (size_t i = 0; i < 3ull * n; i++) if (!std::isfinite(xyz[i])) return fail(c, TB_E_INVALID, std::string(what) + ": a value is not finite");
        Dynamic& d = dynamicOf(c);
        if (!d.ready) makeTables(c, d);
        DevBuf& staged = normals ? d.normals : d.positions;
        if (normals && !staged.p) ensure(staged, std::max<size_t>(16, 12ull * numVertices(c)));
        float* at = (float*)staged.p + 3ull * first;
        if (device) HIP_TRY(refit_launch_stage(c->stream, (float*)staged.p, first, n, xyz));
        else { HIP_TRY(hipMemcpyAsync(at, xyz, bytes, hipMemcpyHostToDevice, c->stream)); HIP_TRY(hipStreamSynchronize(c->stream)); }
        addRange(normals ? d.dirtyNormals : d.dirtyPositions, first, n);
        return TB_OK;
    });
}

/* Which form of the bottom-up pass runs: 0, one launch per level; 1, the top levels fused into one single-workgroup launch.  TB_REFIT_FORM in the
 * environment is the diagnostic of scripts/refit_rate.py, which measures the two against each other in one process; unset, empty or anything else:
 * what ships, kRefitForm -- the fused top, which took 15 to 37 microseconds off a commit on every scene measured, outside the spread of either
 * form's windows (profiles/refit_rate.json). */
constexpr int kRefitForm = 1;
int refitForm()
{
    const char* e = getenv("TB_REFIT_FORM");
    return e && (e[0] == '0' || e[0] == '1') && !e[1] ? e[0] - '0' : kRefitForm;
}

/* the refit on the stream, the root box back */
void refit(tb_context* c, Dynamic& d)
{
    RefitTables t{};
    t.positions = (const float*)d.positions.p; t.triVerts = (const uint32_t*)d.triVerts.p; t.triSlot = (const uint32_t*)d.triSlot.p;
    t.nodeSlot = (const uint32_t*)d.nodeSlot.p; t.schedule = (const uint32_t*)d.schedule.p;
    t.tris = (TbTriB*)c->ds.tris; t.nodes = (TbNodeB*)c->ds.nodes; t.rootBox = (float*)d.rootBox.p;
    t.numTris = c->ds.numTris; t.numNodes = c->ds.numNodes;
    HIP_TRY(hipEventRecord(d.ev[0].create(), c->stream));
    const uint32_t numLevels = (uint32_t)d.levelFirst.size() - 1;
    const uint32_t fusedFirst = refitForm() == 1 ? refit_fused_first_level(d.levelFirst.data(), numLevels) : numLevels;
    HIP_TRY(refit_launch_fit(c->stream, &t, d.levelFirst.data(), numLevels, (const uint32_t*)d.levelFirstDevice.p, fusedFirst));
    HIP_TRY(hipEventRecord(d.ev[1].create(), c->stream));
    float box[6]; /* the one read of a commit: TbDeviceScene travels as a kernel argument */
    HIP_TRY(hipMemcpyAsync(box, d.rootBox.p, sizeof box, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&d.lastMs, d.ev[0], d.ev[1]));
    memcpy(c->ds.rootCenter, box, 12); memcpy(c->ds.rootHalf, box + 3, 12);
    d.refitSinceBuild = true;
}

/* staged instance transforms into the scene, the top level again, its device image rewritten in place */
void applyTransforms(tb_context* c, Dynamic& d)
{
    HostScene& s = c->scene;
    const uint32_t M = (uint32_t)s.instances.size();
    for (uint32_t i = 0; i < M; i++) if (d.transformStaged[i]) {
        memcpy(s.instances[i].objectToWorld, &d.transforms[12ull * i], 48);
        InvertInstanceTransform(s.instances[i].objectToWorld, s.instances[i].worldToObject);
    }
    const int64_t builder = opt<OPT_bvh_builder>(c);
    if (builder == 2 || builder == 4)
        RebuildTopLevel(s, [&](HostScene& all, const std::vector<float>& boxes, std::vector<TbNodeB>& top, uint32_t& rootRef, uint32_t& depth) {
            BuildTlasGpu(c, all, boxes, top, rootRef, depth); });
    else RebuildTopLevel(s, nullptr);
    /* the device forms of finalizeScene: top-level refs address 64-B instance records and 64-B nodes, 4 units each */
    auto topRef = [](uint32_t ref) { return (ref & TB_BVH_LEAF_FLAG) ? (TB_BVH_LEAF_FLAG | ((ref & ~TB_BVH_LEAF_FLAG) * 4u)) : ref * 4u; };
    std::vector<TbNodeB> top(s.nodesB.begin(), s.nodesB.begin() + (M > 1 ? M - 1 : 0));
    for (TbNodeB& nd : top) { nd.left = topRef(nd.left); nd.right = topRef(nd.right); }
    if (!top.empty()) HIP_TRY(hipMemcpyAsync((void*)c->ds.nodes, top.data(), top.size() * sizeof(TbNodeB), hipMemcpyHostToDevice, c->stream));
    std::vector<TbInstanceB> devInst(s.instancesB);
    for (TbInstanceB& ib : devInst) ib.blasRootRef = (ib.blasRootRef & TB_BVH_LEAF_FLAG) ? (TB_BVH_LEAF_FLAG | ((ib.blasRootRef & ~TB_BVH_LEAF_FLAG) * 3u)) :
        ib.blasRootRef * 4u;
    HIP_TRY(hipMemcpyAsync((void*)c->ds.instances, devInst.data(), devInst.size() * sizeof(TbInstanceB), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ds.rootRef = topRef(s.rootRefB);
    const TbAabbNode* root = (const TbAabbNode*)(s.tlasA.data() + 16);
    memcpy(c->ds.rootCenter, root->center, 12); memcpy(c->ds.rootHalf, root->halfDim, 12);
    c->ds.stackDepth = WalkStackDepth(s.bvhMaxDepth);
    /* the scene's bounds: every instance's object-space vertices through its transform (fp32 fma chains, the top level's own arithmetic) */
    float mn[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f}, mx[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
    for (const HostScene::Instance& in : s.instances) {
        const HostScene::Blas& b = s.blas[in.blas];
        for (uint32_t t = 3 * b.firstTri; t < 3 * (b.firstTri + b.numTris); t++) {
            const float* p = &s.positions[3ull * s.triVertexIndex[t]];
            for (int r = 0; r < 3; r++) {
                const float* m = in.objectToWorld + 4 * r;
                const float w = tb_fma(m[2], p[2], tb_fma(m[1], p[1], tb_fma(m[0], p[0], m[3])));
                mn[r] = std::min(mn[r], w); mx[r] = std::max(mx[r], w);
            }
        }
    }
    memcpy(s.sceneMin, mn, 12); memcpy(s.sceneMax, mx, 12);
}

} // namespace

/* The host copies of a one-level scene's geometry from the device: triangles and boxes as they lie there, positions from the triangles, layout A from
 * layout B (the same numbers: both trees are walked from their roots side by side). */
void tbctx::refreshHostScene(tb_context* c)
{
    if (!c->dyn || !c->dyn->hostStale) return;
    Dynamic& d = *c->dyn;
    HostScene& s = c->scene;
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t N = s.trisB.size(), numNodes = s.nodesB.size();
    HIP_TRY(hipMemcpy(s.trisB.data(), c->ds.tris, N * sizeof(TbTriB), hipMemcpyDeviceToHost));
    {
        std::vector<TbNodeB> dev(numNodes);
        HIP_TRY(hipMemcpy(dev.data(), c->ds.nodes, numNodes * sizeof(TbNodeB), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < numNodes; i++) memcpy(&s.nodesB[i], &dev[i], 48); /* the boxes; the host keeps its own child refs */
    }
    if (d.vertexBufferStale) HIP_TRY(hipMemcpy(s.vertexBuffer.data(), c->ds.vertexBuffer, s.vertexBuffer.size() * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < N; k++) {
        const float* v[3] = {s.trisB[k].v0, s.trisB[k].v1, s.trisB[k].v2};
        for (int j = 0; j < 3; j++) memcpy(&s.positions[3ull * d.hostTriVerts[3 * k + j]], v[j], 12);
    }
    tb3 mn = tb3_splat(3.402823466e+38f), mx = tb3_splat(-3.402823466e+38f);
    for (size_t i = 0; i + 2 < s.positions.size(); i += 3) { const tb3 p = tb3_make(s.positions[i], s.positions[i + 1], s.positions[i + 2]);
        mn = tb3_min(mn, p); mx = tb3_max(mx, p); }
    s.sceneMin[0] = mn.x; s.sceneMin[1] = mn.y; s.sceneMin[2] = mn.z; s.sceneMax[0] = mx.x; s.sceneMax[1] = mx.y; s.sceneMax[2] = mx.z;
    /* layout A */
    TbBvhHeader hdr; memcpy(&hdr, s.bvhA.data(), 16);
    TbAabbNode* nodesA = (TbAabbNode*)(s.bvhA.data() + hdr.offsetToBoxes);
    uint8_t* prims = s.bvhA.data() + hdr.offsetToVertices;
    for (size_t k = 0; k < N; k++) { float* p = (float*)(prims + 40ull * k); /* type word, then nine floats */
        memcpy(p + 1, s.trisB[k].v0, 12); memcpy(p + 4, s.trisB[k].v1, 12); memcpy(p + 7, s.trisB[k].v2, 12); }
    memcpy(nodesA[0].center, c->ds.rootCenter, 12); memcpy(nodesA[0].halfDim, c->ds.rootHalf, 12);
    if (!(s.rootRefB & TB_BVH_LEAF_FLAG)) {
        std::vector<std::pair<uint32_t, uint32_t>> st(1, std::make_pair(0u, s.rootRefB)); /* (layout-A node, layout-B node) */
        while (!st.empty()) {
            const uint32_t a = st.back().first, b = st.back().second; st.pop_back();
            const TbNodeB& nb = s.nodesB[b];
            const uint32_t childA[2] = {nodesA[a].flags & TB_BVH_INDEX_MASK, nodesA[a].rightNodeIndex}, childB[2] = {nb.left, nb.right};
            for (int k = 0; k < 2; k++) {
                TbAabbNode& n = nodesA[childA[k]];
                n.center[0] = nb.cx[k]; n.center[1] = nb.cy[k]; n.center[2] = nb.cz[k]; n.halfDim[0] = nb.hx[k]; n.halfDim[1] = nb.hy[k]; n.halfDim[2] = nb.hz[k];
                if (!(childB[k] & TB_BVH_LEAF_FLAG)) st.emplace_back(childA[k], childB[k]);
            }
        }
    }
    d.hostStale = false; d.vertexBufferStale = false;
}

extern "C" {

int tb_update_positions(tb_context* c, uint32_t flags, uint32_t first, uint32_t n, const float* xyz)
{
    return stageVertices(c, "tb_update_positions", false, flags, first, n, xyz);
}

int tb_update_normals(tb_context* c, uint32_t flags, uint32_t first, uint32_t n, const float* xyz)
{
    return stageVertices(c, "tb_update_normals", true, flags, first, n, xyz);
}

int tb_recompute_normals(tb_context* c, uint32_t first, uint32_t n)
{
    TB_REFUSE_PEER(c);
    if (c && !c->group.peers.empty()) return fail(c, TB_E_UNSUPPORTED, "tb_recompute_normals: not supported for a multi-device group");
    return guarded(c, [&]() {
        int code; const float nothing = 0.0f; /* the call brings no array: updateRefusal's pointer test has nothing to refuse */
        if (const char* why = updateRefusal(c, "tb_recompute_normals", 0, first, n, &nothing, code)) return fail(c, code, std::string("tb_recompute_normals: ") + why);
        if (n == 0) return TB_OK;
        Dynamic& d = dynamicOf(c);
        if (!d.ready) makeTables(c, d);
        if (!d.normalTablesReady) makeNormalTables(c, d);
        addRange(d.markedNormals, first, n);
        return TB_OK;
    });
}

int tb_geometry_vertex_range(tb_context* c, uint32_t geometry, uint32_t* first, uint32_t* count)
{
    if (!c || !first || !count) return TB_E_INVALID;
    if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
    if (geometry >= c->scene.hitGroups.size()) return fail(c, TB_E_INVALID, "tb_geometry_vertex_range: geometry out of range");
    vertexRangeOf(c->scene, geometry, *first, *count);
    return TB_OK;
}

int tb_set_instance_transforms(tb_context* c, uint32_t first, uint32_t n, const float* m)
{
    TB_REFUSE_PEER(c);
    if (c && !c->group.peers.empty()) return fail(c, TB_E_UNSUPPORTED, "tb_set_instance_transforms: not supported for a multi-device group");
    return guarded(c, [&]() {
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
        if (!twoLevel(c)) return fail(c, TB_E_UNSUPPORTED, "tb_set_instance_transforms: the scene has no instances (option flatten_instances = 0 keeps them)");
        const uint32_t M = (uint32_t)c->scene.instances.size();
        if ((uint64_t)first + n > M) return fail(c, TB_E_INVALID, "tb_set_instance_transforms: the range runs past the scene's instances");
        if (n && !m) return fail(c, TB_E_INVALID, "tb_set_instance_transforms: null pointer");
        for (uint32_t i = 0; i < n; i++) {
            for (int k = 0; k < 12; k++) if (!std::isfinite(m[12ull * i + k]))
                return fail(c, TB_E_INVALID, "tb_set_instance_transforms: transform " + std::to_string(first + i) + " is not finite");
            const float det = InstanceTransformDeterminant(m + 12ull * i);
            if (!std::isfinite(det) || det == 0.0f || !std::isfinite(1.0f / det))
                return fail(c, TB_E_INVALID, "tb_set_instance_transforms: the 3x3 part of transform " + std::to_string(first + i) + " is singular");
        }
        if (n == 0) return TB_OK;
        Dynamic& d = dynamicOf(c);
        if (d.transforms.empty()) { d.transforms.assign(12ull * M, 0.0f); d.transformStaged.assign(M, 0); }
        memcpy(&d.transforms[12ull * first], m, 48ull * n);
        for (uint32_t i = 0; i < n; i++) d.transformStaged[first + i] = 1;
        return TB_OK;
    });
}

int tb_commit_geometry(tb_context* c, uint32_t flags)
{
    TB_REFUSE_PEER(c);
    if (c && !c->group.peers.empty()) return fail(c, TB_E_UNSUPPORTED, "tb_commit_geometry: not supported for a multi-device group");
    return guarded(c, [&]() {
        if (!c->hasScene) return fail(c, TB_E_NO_SCENE, "no scene loaded");
        if (flags & ~TB_GEOMETRY_REBUILD) return fail(c, TB_E_INVALID, "tb_commit_geometry: unknown flag bits");
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!c->dyn) return TB_OK;
        Dynamic& d = *c->dyn;
        const bool rebuild = (flags & TB_GEOMETRY_REBUILD) != 0;
        bool transforms = false;
        for (uint8_t s : d.transformStaged) transforms = transforms || s != 0;
        mergeRanges(d.dirtyPositions); mergeRanges(d.dirtyNormals); mergeRanges(d.markedNormals);
        const bool vertices = !d.dirtyPositions.empty(), marks = !d.markedNormals.empty(), normals = !d.dirtyNormals.empty() || marks;
        if (!vertices && !normals && !transforms && !(rebuild && d.refitSinceBuild)) return TB_OK;
        if (rebuild && twoLevel(c)) return fail(c, TB_E_UNSUPPORTED, "tb_commit_geometry: TB_GEOMETRY_REBUILD of a two-level scene is not supported");
        int g = movedEmissiveGeometry(c, d.dirtyPositions, d.positions, false);
        if (g < 0) g = movedEmissiveGeometry(c, d.dirtyNormals, d.normals, true);
        if (g >= 0) return fail(c, TB_E_UNSUPPORTED, "tb_commit_geometry: geometry " + std::to_string(g) +
            " has an emissive material and staged vertices of it have changed: its lights are not made again");
        if (transforms) { applyTransforms(c, d); std::fill(d.transformStaged.begin(), d.transformStaged.end(), 0); }
        if (vertices) refit(c, d);
        for (const auto& r : d.dirtyNormals)
            HIP_TRY(refit_launch_normals(c->stream, (float*)c->ds.vertexBuffer, (const float*)d.normals.p, r.first, r.second - r.first));
        if (marks) recomputeNormals(c, d, vertices); /* last: a recomputation wins over an explicit normal of the same vertex */
        if (normals) { HIP_TRY(hipStreamSynchronize(c->stream)); d.vertexBufferStale = true; }
        if (vertices || normals) d.hostStale = true;
        d.dirtyPositions.clear(); d.dirtyNormals.clear(); d.markedNormals.clear();
        if (rebuild) {   /* what a fresh load of the moved scene builds: the host positions, then finalizeScene, which drops this state with the scene's buffers */
            refreshHostScene(c);
            const tb_camera camera = c->camera;
            finalizeScene(c, true);
            c->camera = camera;
            return TB_OK;
        }
        if (vertices) {
            dropCompactNodes(c); /* its quantisation frame is the root box: ensureCompactNodes makes it again */
            if (c->sceneInLds && c->ds.ldsBlob) {
                refreshHostScene(c);
                const LdsImage image = BuildLdsImage(c->scene.nodesB.data(), c->scene.nodesB.size(), c->scene.trisB.data(), c->scene.trisB.size());
                if (image.bytes.size() != c->ds.ldsBlobBytes) throw std::runtime_error("dynamic geometry: the LDS image changed its size");
                HIP_TRY(hipMemcpy((void*)c->ds.ldsBlob, image.bytes.data(), image.bytes.size(), hipMemcpyHostToDevice));
            }
        }
        sceneChanged(c);
        return TB_OK;
    });
}

} // extern "C"
