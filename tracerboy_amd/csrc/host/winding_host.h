/* winding_host.h -- the rule of include/tb_winding.h as scalar C++ over a layout-B tree with HOST child refs (indices): the moments of every subtree,
 * the exact sum over every triangle in order, and wn_kernels.hip's depth-first walk.  Shared by host_api.cpp (tb_host_scene_winding) and
 * context_winding.cpp (tb_winding_numbers with TB_WINDING_HOST_WALK, over the context's own host copies); needs no device and no HIP header. */
#pragma once
#include "tb_abi.h"
#include "tb_winding.h"

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <thread>
#include <utility>
#include <vector>

namespace tbwinding {

struct Tree { const TbNodeB* nodes; size_t numNodes; const TbTriB* tris; size_t numTris; uint32_t rootRef; };
struct Moments { std::vector<TbMoments> child; TbMoments root; }; /* child[2 * node + side] */

inline tb3 corner(const float* v) { return tb3_make(v[0], v[1], v[2]); }
inline TbMoments leafMoments(const TbTriB& t) { return tb_moments_leaf(corner(t.v0), corner(t.v1), corner(t.v2)); }
inline float solidAngle(tb3 p, const TbTriB& t) { return tb_solid_angle(p, corner(t.v0), corner(t.v1), corner(t.v2)); }

/* every subtree's moments, children before parents (a pre-order list read backwards) */
inline Moments fit(const Tree& t)
{
    Moments m; m.child.assign(2 * t.numNodes, TbMoments{});
    auto leaf = [&](uint32_t ref) { const uint32_t i = ref & ~TB_BVH_LEAF_FLAG; if (i >= t.numTris) throw std::runtime_error("winding: a leaf is out of range");
        return leafMoments(t.tris[i]); };
    if (t.rootRef & TB_BVH_LEAF_FLAG) { m.root = leaf(t.rootRef); return m; }
    if (t.rootRef >= t.numNodes) throw std::runtime_error("winding: the root is out of range");
    std::vector<uint32_t> order, st(1, t.rootRef);
    while (!st.empty()) {
        const uint32_t x = st.back(); st.pop_back(); order.push_back(x);
        if (order.size() > t.numNodes) throw std::runtime_error("winding: the tree is not a tree");
        for (uint32_t r : {t.nodes[x].left, t.nodes[x].right}) if (!(r & TB_BVH_LEAF_FLAG)) { if (r >= t.numNodes) throw std::runtime_error("winding: a node is out of range");
            st.push_back(r); }
    }
    for (size_t k = order.size(); k-- > 0;) {
        const uint32_t x = order[k], to[2] = {t.nodes[x].left, t.nodes[x].right};
        for (int s = 0; s < 2; s++)
            m.child[2ull * x + s] = (to[s] & TB_BVH_LEAF_FLAG) ? leaf(to[s]) : tb_moments_parent(m.child[2ull * to[s]], m.child[2ull * to[s] + 1]);
    }
    m.root = tb_moments_parent(m.child[2ull * t.rootRef], m.child[2ull * t.rootRef + 1]);
    return m;
}

/* the exact form over the array's order */
inline float brute(const Tree& t, tb3 p)
{
    if (!tb_winding_finite3(p)) return tb_u2f(TB_WINDING_NAN);
    float acc = 0.0f;
    for (size_t k = 0; k < t.numTris; k++) acc = acc + solidAngle(p, t.tris[k]);
    return acc * TB_WINDING_INV_4PI;
}

/* the kernel's walk, one point.  stack: (node, side) visits still due */
inline float walk(const Tree& t, const Moments& m, tb3 p, float beta, std::vector<std::pair<uint32_t, uint32_t>>& stack)
{
    if (!tb_winding_finite3(p)) return tb_u2f(TB_WINDING_NAN);
    float acc = 0.0f;
    /* one subtree: true, nothing below it is left to do */
    auto offer = [&](const TbMoments& s, uint32_t ref) {
        const tb3 d = s.c - p;
        const float L2 = tb3_dot(d, d);
        if (tb_winding_accepts(L2, s.r, beta)) { acc = acc + tb_winding_dipole(s.N, d, L2); return true; }
        if (ref & TB_BVH_LEAF_FLAG) { acc = acc + solidAngle(p, t.tris[ref & ~TB_BVH_LEAF_FLAG]); return true; }
        return false;
    };
    stack.clear();
    if (!offer(m.root, t.rootRef)) stack.emplace_back(t.rootRef, 0u);
    while (!stack.empty()) {
        const uint32_t node = stack.back().first; uint32_t side = stack.back().second; stack.pop_back();
        for (; side < 2; side++) {
            const uint32_t ref = side ? t.nodes[node].right : t.nodes[node].left;
            if (offer(m.child[2ull * node + side], ref)) continue;
            if (!side) stack.emplace_back(node, 1u);
            stack.emplace_back(ref, 0u);
            break;
        }
    }
    return acc * TB_WINDING_INV_4PI;
}

/* w of n points into out; a point's number depends on nothing but the point, so a large job is dealt over a few threads by point */
inline void run(const Tree& t, bool useWalk, uint64_t n, const TbQueryPoint* points, float beta, float* out)
{
    Moments m;
    if (useWalk) m = fit(t);
    auto range = [&](uint64_t first, uint64_t end) {
        std::vector<std::pair<uint32_t, uint32_t>> stack;
        for (uint64_t i = first; i < end; i++) {
            const tb3 p = corner(points[i].Position);
            out[i] = useWalk ? walk(t, m, p, beta, stack) : brute(t, p);
        }
    };
    const uint64_t work = useWalk ? n * 256u : n * (uint64_t)t.numTris * 4u;
    const uint64_t threads = work < (1ull << 22) ? 1u : std::min<uint64_t>(std::min<uint64_t>(8u, std::max(1u, std::thread::hardware_concurrency())), n);
    std::vector<std::thread> pool;
    uint64_t k = 0;
    try { for (; k + 1 < threads; k++) pool.emplace_back(range, n * k / threads, n * (k + 1) / threads); } catch (const std::exception&) {}
    range(n * k / threads, n); /* the calling thread takes the last share, and what no thread could be started for */
    for (std::thread& th : pool) th.join();
}

} // namespace tbwinding
