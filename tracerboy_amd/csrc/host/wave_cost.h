/* wave_cost.h -- what a 64-lane wave pays to walk a tree, as pure host functions: no context, no device.  The reinsertion passes of builder 1
 * minimise what a random single ray pays (summed inner-node area); a lock-step wave pays for its longest lane.  Three pieces, used by the
 * wave stage of bvh_build.cpp and exported through host_api.cpp for the CPU tests:
 *   - WaveWalk: one ray over a WaveTree with the kernels' rule (traverse(), pt_device.hpp; Traverse(), oracle/tb_oracle.cpp): root box test, both
 *     children tested when a node is visited, near child first (rt < lt goes right, ties go left), far child parked, `closest` tightened by every
 *     accepted triangle, the degenerate-axis constants and the NaN rule.  It appends the ray's steps, 'I' per inner node visited and 'L' per triangle
 *     tested, as the oracle's ray log writes them.  The arithmetic is tb_vec.h / tb_math.h's, so the visits are the oracle's;
 *   - WaveReplay: up to 64 step strings under the schedule of the LDS steps (pt_device.hpp, LDS_STEPS): the inner loop runs while at least parkMin
 *     lanes descend, then one leaf pass; a pass whose leaf step no lane takes is counted as idle (the last pass of every walk is one);
 *   - WaveModelRays: a deterministic ray set made from the scene's triangles alone, by an integer hash.
 * Cost = inner trips x kWaveInnerInsts + leaf trips x kWaveLeafInsts: the wave instructions of one trip through the inner loop and through the leaf
 * step of pt_persistent<0, SCENE_LDS, !COUNT, GROUPS> in pt_variant_matte6.hip, as scripts/isa_walk_steps.py counts them (63 and 88). */
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "../../../include/tb_vec.h"

namespace tbhost {

constexpr uint32_t kWaveInnerInsts = 63, kWaveLeafInsts = 88;
constexpr float kWaveMinT = 0.001f, kWaveMaxT = 999999.0f; /* MIN_T and the closest-hit walk's TMax (oracle/tb_oracle.cpp) */
constexpr uint32_t kWaveLanes = 64;

/* What a walk reads of a tree: inner nodes 0 .. N-2 with the root at 0, leaf k at node N-1+k; boxes as centre and half extent, children in the
 * order of the image (the smaller subtree on the left) */
struct WaveTree {
    uint32_t N = 0;
    std::vector<tb3> center, half;     /* 2N - 1 */
    std::vector<uint32_t> left, right; /* N - 1 */
    std::vector<tb3> v0, v1, v2;       /* N: leaf k's triangle */
};

/* Boxes and child order from a topology and the leaves' bounds, with the arithmetic of the image (bvh_build.cpp BuildBvhSingle: the 0.001 thin-box
 * padding, centre = (min + max) / 2, half = max - centre, an inner box from its children's centre -+ half, the child with fewer triangles on the
 * left).  left / right: the builder's children of inner node i.  Returns the tree's depth in nodes.  The triangles stay as they are. */
inline uint32_t WaveTreeFit(WaveTree& w, uint32_t N, const uint32_t* left, const uint32_t* right, const tb3* leafMin, const tb3* leafMax)
{
    w.N = N;
    if (!N) return 0;
    const uint32_t M = 2 * N - 1;
    w.center.resize(M); w.half.resize(M); w.left.resize(N - 1); w.right.resize(N - 1);
    auto put = [&](uint32_t i, tb3 mn, tb3 mx) { const tb3 c = (mn + mx) * 0.5f; w.center[i] = c; w.half[i] = mx - c; };
    std::vector<uint32_t> walk, depth(M, 0), count(M, 0), st; walk.reserve(M);
    st.push_back(0); depth[0] = 1; uint32_t maxD = 1;
    while (!st.empty()) { const uint32_t x = st.back(); st.pop_back(); walk.push_back(x);
        if (x < N - 1) { const uint32_t l = left[x], r = right[x]; depth[l] = depth[r] = depth[x] + 1; maxD = std::max(maxD, depth[l]); st.push_back(l);
            st.push_back(r); } }
    for (size_t k = walk.size(); k-- > 0;) {
        const uint32_t x = walk[k];
        if (x >= N - 1) { const tb3 mx = leafMax[x - (N - 1)], mn = tb3_min(leafMin[x - (N - 1)], mx - tb3_splat(0.001f)); put(x, mn, mx); count[x] = 1; }
        else {
            uint32_t l = left[x], r = right[x];
            if (count[l] > count[r]) std::swap(l, r);
            put(x, tb3_min(w.center[l] - w.half[l], w.center[r] - w.half[r]), tb3_max(w.center[l] + w.half[l], w.center[r] + w.half[r]));
            w.left[x] = l; w.right[x] = r; count[x] = count[l] + count[r];
        }
    }
    return maxD;
}

/* a ray and what GetRayData makes of it (oracle/tb_oracle.cpp; ray_prepare, pt_device.hpp) */
struct WaveRay {
    tb3 o, d; float tMax;
    tb3 inv, oinv, ainv, shear; int kx, ky, kz; bool cannotHit;
};

inline void WaveRayPrepare(WaveRay& r)
{
    const tb3 o = r.o, d = r.d;
    r.cannotHit = tb_isnan(o.x) || tb_isnan(o.y) || tb_isnan(o.z) || tb_isnan(d.x) || tb_isnan(d.y) || tb_isnan(d.z);
    const float DEGEN_INV = 1.2089258196146292e24f, DEGEN_AINV = 1.2101064112353466e24f; /* 2^80 and 2^80 (1 + 2^-10) */
    r.inv = tb3_make(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    r.oinv = o * r.inv;
    const tb3 a = tb3_abs(d);
    const int z = (a.x > a.y && a.x > a.z) ? 0 : (a.y > a.z ? 1 : 2);
    r.kx = (z + 1) % 3; r.ky = (z + 2) % 3; r.kz = z;
    r.ainv = tb3_abs(r.inv);
    if (d.x == 0.0f) { r.inv.x = DEGEN_INV; r.ainv.x = DEGEN_AINV; r.oinv.x = o.x * DEGEN_INV; }
    if (d.y == 0.0f) { r.inv.y = DEGEN_INV; r.ainv.y = DEGEN_AINV; r.oinv.y = o.y * DEGEN_INV; }
    if (d.z == 0.0f) { r.inv.z = DEGEN_INV; r.ainv.z = DEGEN_AINV; r.oinv.z = o.z * DEGEN_INV; }
    if (tb3_get(d, r.kz) < 0.0f) std::swap(r.kx, r.ky);
    r.shear = tb3_make(tb3_get(d, r.kx) / tb3_get(d, r.kz), tb3_get(d, r.ky) / tb3_get(d, r.kz), 1.0f / tb3_get(d, r.kz));
}

/* the part of the box test that `closest` has no hand in: where the ray enters the box (not before its origin) and where it leaves */
inline void WaveBoxSlabs(float& enterT, float& leaveT, const WaveRay& r, tb3 c, tb3 h)
{
    const tb3 mid = tb3_make(tb_fma(c.x, r.inv.x, -r.oinv.x), tb_fma(c.y, r.inv.y, -r.oinv.y), tb_fma(c.z, r.inv.z, -r.oinv.z));
    const tb3 maxL = tb3_make(tb_fma(h.x, r.ainv.x, mid.x), tb_fma(h.y, r.ainv.y, mid.y), tb_fma(h.z, r.ainv.z, mid.z));
    const tb3 minL = tb3_make(tb_fma(-h.x, r.ainv.x, mid.x), tb_fma(-h.y, r.ainv.y, mid.y), tb_fma(-h.z, r.ainv.z, mid.z));
    const float minT = tb_max(tb_max(minL.x, minL.y), minL.z);
    leaveT = tb_min(tb_min(maxL.x, maxL.y), maxL.z);
    enterT = tb_max(minT, 0.0f);
}
inline bool WaveBoxTest(float& resultT, float closest, const WaveRay& r, tb3 c, tb3 h)
{
    float leaveT;
    WaveBoxSlabs(resultT, leaveT, r, c, h);
    return resultT < tb_min(leaveT, closest);
}
/* How a walk tests the box of node n: WaveBoxDirect works it out; the wave stage's search (bvh_build.cpp) has one that remembers, per ray, where
 * the ray enters and leaves every box of the tree it compares with */
struct WaveBoxDirect {
    bool operator()(float& resultT, float closest, const WaveTree& t, const WaveRay& r, uint32_t n) const { return WaveBoxTest(resultT, closest, r, t.center[n], t.half[n]); }
};

/* the watertight test, two-sided; hitT comes in as `closest` and goes out as the candidate's t where one is found */
inline void WaveTriTest(float& hitT, const WaveRay& r, tb3 v0, tb3 v1, tb3 v2)
{
    const tb3 a0 = v0 - r.o, b0 = v1 - r.o, c0 = v2 - r.o;
    float Ax = tb3_get(a0, r.kx), Ay = tb3_get(a0, r.ky), Az = tb3_get(a0, r.kz);
    float Bx = tb3_get(b0, r.kx), By = tb3_get(b0, r.ky), Bz = tb3_get(b0, r.kz);
    float Cx = tb3_get(c0, r.kx), Cy = tb3_get(c0, r.ky), Cz = tb3_get(c0, r.kz);
    Ax = tb_fma(-r.shear.x, Az, Ax); Ay = tb_fma(-r.shear.y, Az, Ay);
    Bx = tb_fma(-r.shear.x, Bz, Bx); By = tb_fma(-r.shear.y, Bz, By);
    Cx = tb_fma(-r.shear.x, Cz, Cx); Cy = tb_fma(-r.shear.y, Cz, Cy);
    const float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    const float det = U + V + W;
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return;
    if (det == 0.0f) return;
    Az = r.shear.z * Az; Bz = r.shear.z * Bz; Cz = r.shear.z * Cz;
    const float T = tb_fma(W, Cz, tb_fma(V, Bz, U * Az));
    float sT = tb_abs(T);
    if ((T > 0.0f) != (det > 0.0f)) sT = -sT;
    if (sT < 0.0f || sT > hitT * tb_abs(det)) return;
    hitT = T * (1.0f / det);
}

constexpr int kWaveWalkStack = 256; /* the oracle's */

/* A set of inner nodes in 128 bits (the wave stage's search, bvh_build.cpp: which nodes a ray visited, which nodes a move changed).  Nodes 0 .. 127
 * have a bit each; a node beyond them sets every bit, so that two sets which both hold such a node always meet: a scene of more than 129 triangles
 * loses the shortcut, never the answer. */
inline void WaveMaskSet(uint64_t mask[2], uint32_t node) { if (node < 128u) mask[node >> 6] |= 1ull << (node & 63u); else mask[0] = mask[1] = ~0ull; }

/* A walk written down so that it can be checked against another tree and taken up in the middle (the wave stage's search): per inner node visited
 * the node, the stack below it (`top` entries from stacks[rest]), the steps the ray had taken before, `closest` as it stood, and what the node put
 * on the stack: the child walked first and the child parked (WavePushes).  A walk is made of nothing else: the stack, `closest`, and at every node
 * popped what that node puts on the stack -- so where another tree's node puts the same two there from the same `closest`, the walk goes on as it
 * did, whatever else differs between the trees. */
constexpr uint32_t kWaveNoNode = 0xffffffffu;
struct WaveVisit { uint32_t node, rest, top, step; float closest; uint32_t first, parked; };
struct WaveRecord { std::vector<WaveVisit> visits; std::vector<uint32_t> stacks; };

/* both children tested, near child first (rt < lt goes right, ties go left), far child parked */
template <class Box>
inline void WavePushesWith(const Box& box, const WaveTree& t, const WaveRay& r, uint32_t node, float closest, uint32_t& first, uint32_t& parked)
{
    const uint32_t l = t.left[node], rr = t.right[node];
    float lt, rt;
    const bool lh = box(lt, closest, t, r, l), rh = box(rt, closest, t, r, rr);
    if (lh && rh) { const bool rightFirst = rt < lt; first = rightFirst ? rr : l; parked = rightFirst ? l : rr; }
    else { first = lh ? l : (rh ? rr : kWaveNoNode); parked = kWaveNoNode; }
}

/* the walk from a given state: `top` entries on `stack` (room for kWaveWalkStack), `closest`; stepBase: where this ray's steps begin in `steps` */
template <class Box>
inline float WaveWalkOnWith(const Box& box, const WaveTree& t, const WaveRay& r, uint32_t* stack, int top, float closest, std::vector<char>& steps,
    size_t stepBase, uint64_t* visited, WaveRecord* rec)
{
    while (top) {
        const uint32_t node = stack[--top];
        if (node >= t.N - 1) {
            steps.push_back('L');
            const uint32_t k = node - (t.N - 1);
            float t0 = closest;
            WaveTriTest(t0, r, t.v0[k], t.v1[k], t.v2[k]);
            if (t0 < closest && t0 > kWaveMinT) closest = t0;
        } else {
            uint32_t first, parked;
            WavePushesWith(box, t, r, node, closest, first, parked);
            if (rec) { rec->visits.push_back(WaveVisit{node, (uint32_t)rec->stacks.size(), (uint32_t)top, (uint32_t)(steps.size() - stepBase), closest, first, parked});
                rec->stacks.insert(rec->stacks.end(), stack, stack + top); }
            steps.push_back('I');
            if (visited) WaveMaskSet(visited, node);
            if (top + 2 > kWaveWalkStack) return closest;
            if (parked != kWaveNoNode) stack[top++] = parked;
            if (first != kWaveNoNode) stack[top++] = first;
        }
    }
    return closest;
}
inline float WaveWalkOn(const WaveTree& t, const WaveRay& r, uint32_t* stack, int top, float closest, std::vector<char>& steps, size_t stepBase,
    uint64_t* visited, WaveRecord* rec)
{
    return WaveWalkOnWith(WaveBoxDirect{}, t, r, stack, top, closest, steps, stepBase, visited, rec);
}


/* The ray's steps, appended to `steps`; the return value is the closest accepted t, r.tMax where nothing was hit.  visited (may be null): the inner
 * nodes the walk visits are added to this WaveMaskSet set; rec (may be null): the visits are appended to this record. */
inline float WaveWalk(const WaveTree& t, const WaveRay& r, std::vector<char>& steps, uint64_t* visited = nullptr, WaveRecord* rec = nullptr)
{
    const float closest = r.tMax;
    if (!t.N || r.cannotHit) return closest;
    float unusedT;
    if (!WaveBoxTest(unusedT, closest, r, t.center[0], t.half[0])) return closest;
    uint32_t stack[kWaveWalkStack]; stack[0] = 0;
    return WaveWalkOn(t, r, stack, 1, closest, steps, steps.size(), visited, rec);
}


struct WaveTrips {
    uint64_t inner = 0, leaf = 0, idle = 0;         /* wave trips through the inner loop's body, leaf passes a lane takes, passes none takes */
    uint64_t innerActive = 0, leafActive = 0;       /* lanes active in them */
    double cost() const { return (double)inner * kWaveInnerInsts + (double)leaf * kWaveLeafInsts; }
    void add(const WaveTrips& o) { inner += o.inner; leaf += o.leaf; idle += o.idle; innerActive += o.innerActive; leafActive += o.leafActive; }
};

/* `lanes` (at most 64) step strings, string l = steps[l] of length len[l], under the LDS steps' schedule:
 *     inner = lanes at an inner node
 *     do { if (inner) do { those lanes take a step } while (popc(inner) >= parkMin);
 *          busy = inner | lanes at a leaf;  the lanes at a leaf take theirs } while (busy)                                                          */
inline WaveTrips WaveReplay(const char* const* steps, const uint32_t* len, uint32_t lanes, uint32_t parkMin)
{
    WaveTrips w;
    if (lanes > kWaveLanes) lanes = kWaveLanes;
    if (parkMin < 1) parkMin = 1;
    /* the lanes at an inner node and at a leaf as bit sets, kept up as the lanes step (the wave stage's search replays some 10^5 waves: only the
     * lanes that step are touched); a lane at its string's end, or at any other character, is in neither and steps no more */
    uint32_t p[kWaveLanes] = {};
    uint64_t inner = 0, leaf = 0;
    auto arrive = [&](uint32_t l) { if (p[l] < len[l]) { const char c = steps[l][p[l]]; if (c == 'I') inner |= 1ull << l; else if (c == 'L') leaf |= 1ull << l; } };
    auto step = [&](uint64_t& set) { uint64_t m = set; set = 0; while (m) { const uint32_t l = (uint32_t)__builtin_ctzll(m); m &= m - 1; p[l]++; arrive(l); } };
    for (uint32_t l = 0; l < lanes; l++) arrive(l);
    bool busy;
    do {
        if (inner) do {
            w.inner++; w.innerActive += (uint64_t)__builtin_popcountll(inner);
            step(inner);
        } while ((uint32_t)__builtin_popcountll(inner) >= parkMin);
        busy = inner != 0 || leaf != 0;
        if (leaf) { w.leaf++; w.leafActive += (uint64_t)__builtin_popcountll(leaf); step(leaf); }
        else w.idle++;
    } while (busy);
    return w;
}

/* ---- model rays ------------------------------------------------------------------------------------------------------------------------------
 * The builder has no picture, so the rays come from the surfaces: points spread by area over the triangles that do not emit, pushed off the surface
 * along the geometric normal (either side, by the hash: a wall seen from outside gives rays that miss the root box, the idle lanes of a wave), from
 * there a cosine-weighted direction (a bounce ray) or a uniform point on a light's triangle (a feeler).  Rays come in waves
 * of 64 of one kind, `feelerPercent` of the waves feelers.  Every number is a function of (seed, ray index) through an integer hash, the
 * trigonometry tb_math.h's: the same rays on every machine. */
struct WaveSurfaces {
    std::vector<tb3> v;            /* three per triangle */
    std::vector<uint8_t> emits;    /* per triangle */
    std::vector<tb3> light;        /* three per light triangle */
};

inline uint32_t WaveHash(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t h = a * 0x9e3779b1u ^ (b + 0x7f4a7c15u) * 0x85ebca6bu ^ (c + 0x165667b1u) * 0xc2b2ae35u;
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
inline float WaveUnit(uint32_t seed, uint32_t index, uint32_t dim) { return (float)(WaveHash(seed, index, dim) >> 8) * (1.0f / 16777216.0f); }

inline void WaveModelRays(const WaveSurfaces& s, uint32_t seed, uint32_t waves, uint32_t feelerPercent, std::vector<WaveRay>& rays)
{
    rays.clear();
    const size_t T = s.v.size() / 3, L = s.light.size() / 3;
    std::vector<double> cdf; std::vector<uint32_t> tri;
    double sum = 0;
    for (size_t i = 0; i < T; i++) {
        if (i < s.emits.size() && s.emits[i]) continue;
        const tb3 n = tb3_cross(s.v[3 * i + 1] - s.v[3 * i], s.v[3 * i + 2] - s.v[3 * i]);
        const double a = 0.5 * std::sqrt((double)n.x * n.x + (double)n.y * n.y + (double)n.z * n.z);
        if (!(a > 0.0)) continue;
        sum += a; cdf.push_back(sum); tri.push_back((uint32_t)i);
    }
    if (tri.empty()) return;
    const uint32_t feelerWaves = L ? (uint32_t)(((uint64_t)waves * feelerPercent + 50u) / 100u) : 0u;
    rays.reserve((size_t)waves * kWaveLanes);
    for (uint32_t wv = 0; wv < waves; wv++) {
        /* feelers spread evenly among the waves (Bresenham) */
        const bool feeler = (uint64_t)(wv + 1) * feelerWaves / waves != (uint64_t)wv * feelerWaves / waves;
        for (uint32_t lane = 0; lane < kWaveLanes; lane++) {
            const uint32_t i = wv * kWaveLanes + lane;
            const double pick = (double)WaveUnit(seed, i, 0) * sum;
            const size_t at = std::min<size_t>((size_t)(std::lower_bound(cdf.begin(), cdf.end(), pick) - cdf.begin()), tri.size() - 1);
            const tb3 a = s.v[3 * tri[at]], b = s.v[3 * tri[at] + 1], c = s.v[3 * tri[at] + 2];
            const float su = tb_sqrt(WaveUnit(seed, i, 1)), u2 = WaveUnit(seed, i, 2);
            const tb3 p = a * (1.0f - su) + b * (su * (1.0f - u2)) + c * (su * u2);
            tb3 n = tb3_normalize(tb3_cross(b - a, c - a));
            if (WaveHash(seed, i, 3) & 1u) n = -n;
            WaveRay r; r.o = p + n * 0.001f; r.tMax = kWaveMaxT;
            if (feeler) {
                const size_t li = (size_t)(WaveHash(seed, i, 4) % (uint32_t)L);
                const float sv = tb_sqrt(WaveUnit(seed, i, 5)), v2 = WaveUnit(seed, i, 6);
                const tb3 q = s.light[3 * li] * (1.0f - sv) + s.light[3 * li + 1] * (sv * (1.0f - v2)) + s.light[3 * li + 2] * (sv * v2);
                const tb3 to = q - r.o; const float dist = tb3_length(to);
                r.d = dist > 0.0f ? to * (1.0f / dist) : n; /* walked like any ray: the kernels' feeler is a closest-hit walk */
            } else {
                /* cosine-weighted about n: a disc sample lifted onto the hemisphere */
                const float e1 = WaveUnit(seed, i, 4), e2 = WaveUnit(seed, i, 5);
                const float rad = tb_sqrt(e1), phi = 6.2831853f * e2;
                const tb3 helper = tb_abs(n.x) < 0.5f ? tb3_make(1, 0, 0) : tb3_make(0, 1, 0);
                const tb3 t1 = tb3_normalize(tb3_cross(helper, n)), t2 = tb3_cross(n, t1);
                r.d = tb3_normalize(t1 * (rad * tb_cos(phi)) + t2 * (rad * tb_sin(phi)) + n * tb_sqrt(tb_max(0.0f, 1.0f - e1)));
            }
            WaveRayPrepare(r);
            rays.push_back(r);
        }
    }
}

/* the model rays, wave by wave, over one tree: trips summed over the waves.  `arena` and `offsets` are scratch the caller keeps between calls */
inline WaveTrips WaveCostOfTree(const WaveTree& t, const std::vector<WaveRay>& rays, uint32_t parkMin, std::vector<char>& arena)
{
    WaveTrips total;
    const char* ptr[kWaveLanes]; uint32_t len[kWaveLanes]; size_t off[kWaveLanes + 1];
    for (size_t first = 0; first < rays.size(); first += kWaveLanes) {
        const uint32_t lanes = (uint32_t)std::min<size_t>(kWaveLanes, rays.size() - first);
        arena.clear();
        for (uint32_t l = 0; l < lanes; l++) { off[l] = arena.size(); WaveWalk(t, rays[first + l], arena); }
        off[lanes] = arena.size();
        const char* base = arena.empty() ? "" : arena.data();
        for (uint32_t l = 0; l < lanes; l++) { ptr[l] = base + off[l]; len[l] = (uint32_t)(off[l + 1] - off[l]); }
        total.add(WaveReplay(ptr, len, lanes, parkMin));
    }
    return total;
}

} // namespace tbhost
