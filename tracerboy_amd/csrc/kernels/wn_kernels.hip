/* wn_kernels.hip -- generalized winding numbers on device buffers (include/tracerboy_hip.h tb_winding_numbers,
 * tb_bake_winding_field, tb_nearest_points_winding, tb_bake_distance_field_winding), by the rule of include/tb_winding.h -- which the host states
 * with the same functions (host/winding_host.h), so the numbers agree on bits.
 *
 * The moments.  One 64-B TbMomentsB record per layout-B node holds both children's (N, centre, radius) and the node's child refs; a node's own
 * moments are stored with its parent ("slot", wn_launch.h), the root's in a buffer of their own, the areas -- which only the fit reads -- in a side
 * array.  wn_fit_leaves writes every leaf's moments from the TbTriB corners; launch h of wn_fit_level takes the nodes of height h of the refit's
 * schedule, whose children's moments lie in their own record, written by earlier launches -- visible at the kernel boundary, with no fence, no
 * counter and no waiting workgroup; wn_fit_top runs the few-node top levels in ONE workgroup with a barrier between them (refit_kernels.hip
 * refit_fit_top has the argument).  One lane per node; nodes of one height never touch the same word.
 *
 * wn_walk_kernel<MODE, GRID>: one point per lane, a depth-first walk of the moment records, left before right.  A lane's `ref` is a visit of child
 * `side` (bit 0; a device node ref is a multiple of 4) of a node, or a leaf whose solid angle is due, or DONE.  At a node (four 16-B loads) the child
 * is accepted (its dipole is added; on to the other child, or a pop), or is a leaf (the lane parks until the wave's leaf step: three 16-B loads,
 * tb_solid_angle), or is descended (the node, side 1, pushed first if the child is the left one).  So a lane adds its contributions in exactly the
 * rule's order, whatever its neighbours do.  The stack is per lane in dynamic LDS, one dword per entry -- a runtime-indexed private array would go to
 * scratch -- and holds at most one entry per level.  No wave waits for another; every loop is bounded by n and by the tree and is left on
 * wave-uniform conditions (ballots), as pq_nearest_kernel's are: the node loop runs while at least parkMin lanes are at nodes.
 * MODE (wn_launch.h): w is written, or decides the sign bit of a distance the unsigned point query left there (a miss, +inf, is not walked). */
#include <hip/hip_runtime.h>
#include "wn_launch.h"
#include "../../../include/tb_winding.h"

namespace {

constexpr int BLOCK = 256;

__device__ __forceinline__ tb3 ld3(const float* p) { return tb3_make(p[0], p[1], p[2]); }

__device__ __forceinline__ void store_moments(const WnTables& t, uint32_t slot, const TbMoments& m)
{
    if (slot == WN_ROOT_SLOT) { float* r = t.root; r[0] = m.N.x; r[1] = m.N.y; r[2] = m.N.z; r[3] = m.c.x; r[4] = m.c.y; r[5] = m.c.z; r[6] = m.r; r[7] = m.area; return; }
    const uint32_t node = slot >> 1, s = slot & 1u;
    if (node >= t.numNodes) return;
    TbMomentsB* o = t.moments + node;
    o->Nx[s] = m.N.x; o->Ny[s] = m.N.y; o->Nz[s] = m.N.z; o->cx[s] = m.c.x; o->cy[s] = m.c.y; o->cz[s] = m.c.z; o->r[s] = m.r;
    t.areas[slot] = m.area;
}

__global__ __launch_bounds__(BLOCK) void wn_fit_leaves(WnTables t)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= t.numTris) return;
    const TbTriB* tri = t.tris + k;
    store_moments(t, t.triSlot[k], tb_moments_leaf(ld3(tri->v0), ld3(tri->v1), ld3(tri->v2)));
}

__device__ __forceinline__ void fit_node(const WnTables& t, uint32_t node)
{
    if (node >= t.numNodes) return;
    TbMomentsB* rec = t.moments + node;
    TbMoments c[2];
    for (int s = 0; s < 2; s++) {
        c[s].N = tb3_make(rec->Nx[s], rec->Ny[s], rec->Nz[s]); c[s].c = tb3_make(rec->cx[s], rec->cy[s], rec->cz[s]); c[s].r = rec->r[s];
        c[s].area = t.areas[2ull * node + s];
    }
    rec->left = t.nodes[node].left; rec->right = t.nodes[node].right; /* this lane alone writes these two words */
    store_moments(t, t.nodeSlot[node], tb_moments_parent(c[0], c[1]));
}

__global__ __launch_bounds__(BLOCK) void wn_fit_level(WnTables t, uint32_t first, uint32_t count)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < count) fit_node(t, t.schedule[first + i]);
}

__global__ __launch_bounds__(BLOCK) void wn_fit_top(WnTables t, const uint32_t* levelFirst, uint32_t firstLevel, uint32_t numLevels)
{
    for (uint32_t l = firstLevel; l < numLevels; l++) {
        const uint32_t end = levelFirst[l + 1];
        for (uint32_t i = levelFirst[l] + threadIdx.x; i < end; i += BLOCK) fit_node(t, t.schedule[i]);
        __syncthreads();
    }
}

struct WnWalkArgs {
    const uint4* moments; const uint4* tris; const float* root;
    uint32_t rootRef, parkMin, stackDepth, n;
    const TbQueryPoint* points; tb_probe_grid grid; float beta; void* out;
};

template <int MODE, bool GRID>
__global__ __launch_bounds__(BLOCK) void wn_walk_kernel(WnWalkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* const stack = (uint32_t*)smem + threadIdx.x;
    constexpr uint32_t DONE = 0xffffffffu;  /* has the leaf bit: an idle lane takes no node step */
    constexpr uint32_t POP = 0xfffffffeu;   /* `after`: the leaf was a right child, or the root */
    const int parkMin = (int)a.parkMin > 1 ? (int)a.parkMin : 1;
    const float beta = a.beta;
    const uint32_t index = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t ref = DONE, after = POP, top = 0;
    tb3 p = tb3_splat(0.0f);
    float acc = 0.0f, distance = 0.0f;
    bool finite = false, wanted = false;
    if (index < a.n) {
        if (GRID) {
            const uint32_t ci = index % a.grid.count[0], rest = index / a.grid.count[0], cj = rest % a.grid.count[1], ck = rest / a.grid.count[1];
            p = ld3(a.grid.origin) + tb3_make((float)ci, (float)cj, (float)ck) * ld3(a.grid.spacing);
        } else {
            const uint4 q = *(const uint4*)(a.points + index); /* 16 B, 16-B aligned: one load; MaxDistance is not read */
            p = tb3_make(__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z));
        }
        finite = tb_winding_finite3(p);
        wanted = finite;
        if (MODE == WN_SIGN_RECORDS) { distance = ((const TbNearest*)a.out)[index].Distance; wanted = finite && distance != tb_u2f(0x7f800000u); }
        if (MODE == WN_SIGN_CELLS) { distance = ((const float*)a.out)[index]; wanted = finite && distance != tb_u2f(0x7f800000u); }
        if (wanted) { /* the root's own moments first */
            const tb3 d = ld3(a.root + 3) - p;
            const float L2 = tb3_dot(d, d);
            if (tb_winding_accepts(L2, a.root[6], beta)) acc = acc + tb_winding_dipole(ld3(a.root), d, L2);
            else ref = a.rootRef; /* a leaf: its solid angle is due; a node: its side 0 */
        }
    }
    auto pop = [&]() -> uint32_t { return top ? stack[--top * BLOCK] : DONE; };
    for (;;) {
        unsigned long long atNode = __ballot(!(ref & TB_BVH_LEAF_FLAG));
        const unsigned long long atLeaf = __ballot(ref != DONE && (ref & TB_BVH_LEAF_FLAG));
        if ((atNode | atLeaf) == 0ull) break;
        if (atNode != 0ull) {
            do {
                if (!(ref & TB_BVH_LEAF_FLAG)) {
                    const uint32_t node = ref & ~3u;
                    const uint4* rec = a.moments + node;
                    const uint4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
                    /* the visit of child s: true, it was accepted and the walk goes on past it */
                    auto child = [&](bool s) -> bool {
                        const tb3 N = tb3_make(__uint_as_float(s ? q0.y : q0.x), __uint_as_float(s ? q0.w : q0.z), __uint_as_float(s ? q1.y : q1.x));
                        const tb3 c = tb3_make(__uint_as_float(s ? q1.w : q1.z), __uint_as_float(s ? q2.y : q2.x), __uint_as_float(s ? q2.w : q2.z));
                        const float r = __uint_as_float(s ? q3.y : q3.x);
                        const uint32_t to = s ? q3.w : q3.z;
                        const tb3 d = c - p;
                        const float L2 = tb3_dot(d, d);
                        if (tb_winding_accepts(L2, r, beta)) { acc = acc + tb_winding_dipole(N, d, L2); return true; }
                        if (to & TB_BVH_LEAF_FLAG) { ref = to; after = s ? POP : (node | 1u); return false; }
                        if (!s && top < a.stackDepth) { stack[top * BLOCK] = node | 1u; top++; }
                        ref = to;
                        return false;
                    };
                    if ((ref & 1u) || child(false)) { if (child(true)) ref = pop(); }
                }
                atNode = __ballot(!(ref & TB_BVH_LEAF_FLAG));
            } while (__popcll(atNode) >= parkMin);
        }
        if (ref != DONE && (ref & TB_BVH_LEAF_FLAG)) {
            const uint4* tri = a.tris + (ref & TB_DEVICE_REF_MASK);
            const uint4 t0 = tri[0], t1 = tri[1], t2 = tri[2];
            acc = acc + tb_solid_angle(p, tb3_make(__uint_as_float(t0.x), __uint_as_float(t0.y), __uint_as_float(t0.z)),
                tb3_make(__uint_as_float(t1.x), __uint_as_float(t1.y), __uint_as_float(t1.z)), tb3_make(__uint_as_float(t2.x), __uint_as_float(t2.y), __uint_as_float(t2.z)));
            ref = after == POP ? pop() : after;
            after = POP;
        }
    }
    if (index >= a.n) return;
    const float w = finite ? acc * TB_WINDING_INV_4PI : tb_u2f(TB_WINDING_NAN);
    if (MODE == WN_WRITE) { ((float*)a.out)[index] = w; return; }
    if (!wanted || !tb_winding_inside(w)) return;
    if (MODE == WN_SIGN_RECORDS) ((TbNearest*)a.out)[index].Distance = -distance;
    else ((float*)a.out)[index] = -distance;
}

bool wn_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1u)) == 0; }
inline uint32_t blocksFor(uint64_t n) { return (uint32_t)((n + BLOCK - 1) / BLOCK); }

template <class K> hipError_t wn_launch(K kernel, hipStream_t stream, const TbDeviceScene* ds, const TbMomentsB* moments, const float* root, uint32_t n,
    const TbQueryPoint* points, const tb_probe_grid& grid, float beta, void* out)
{
    if (!ds || !moments || !root || !n || n > 0x80000000u || ds->numInstances || !ds->numTris || !(beta >= 1.0f)) return hipErrorInvalidValue;
    WnWalkArgs a{};
    a.moments = (const uint4*)moments; a.tris = (const uint4*)ds->tris; a.root = root;
    a.rootRef = ds->rootRef; a.parkMin = ds->parkMin; a.stackDepth = ds->stackDepth > 0 ? ds->stackDepth : 1u; a.n = n;
    a.points = points; a.grid = grid; a.beta = beta; a.out = out;
    const size_t lds = (size_t)a.stackDepth * BLOCK * 4;
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocksFor(n)), dim3(BLOCK), lds, stream, a);
    return hipGetLastError();
}

} // namespace

extern "C" hipError_t wn_launch_fit(hipStream_t stream, const WnTables* t, const uint32_t* levelFirst, uint32_t numLevels, const uint32_t* levelFirstDevice,
    uint32_t fusedFirstLevel)
{
    if (!t->numTris) return hipSuccess;
    (void)hipGetLastError(); /* sticky: an error an earlier call left unread is not this launch's */
    hipLaunchKernelGGL(wn_fit_leaves, dim3(blocksFor(t->numTris)), dim3(BLOCK), 0, stream, *t);
    const uint32_t chained = fusedFirstLevel < numLevels ? fusedFirstLevel : numLevels;
    for (uint32_t l = 0; l < chained; l++) {
        const uint32_t first = levelFirst[l], count = levelFirst[l + 1] - first;
        if (!count) continue;
        hipLaunchKernelGGL(wn_fit_level, dim3(blocksFor(count)), dim3(BLOCK), 0, stream, *t, first, count);
    }
    if (chained < numLevels) hipLaunchKernelGGL(wn_fit_top, dim3(1), dim3(BLOCK), 0, stream, *t, levelFirstDevice, chained, numLevels);
    return hipGetLastError();
}

extern "C" hipError_t wn_launch_points(hipStream_t stream, const TbDeviceScene* ds, const TbMomentsB* moments, const float* root, int mode, uint32_t n,
    const TbQueryPoint* points, float beta, void* out)
{
    if (!wn_aligned(points, 16) || !wn_aligned(out, mode == WN_SIGN_RECORDS ? 16 : 4)) return hipErrorInvalidValue;
    if (mode == WN_WRITE) return wn_launch(wn_walk_kernel<WN_WRITE, false>, stream, ds, moments, root, n, points, tb_probe_grid{}, beta, out);
    if (mode == WN_SIGN_RECORDS) return wn_launch(wn_walk_kernel<WN_SIGN_RECORDS, false>, stream, ds, moments, root, n, points, tb_probe_grid{}, beta, out);
    return hipErrorInvalidValue;
}

extern "C" hipError_t wn_launch_grid(hipStream_t stream, const TbDeviceScene* ds, const TbMomentsB* moments, const float* root, int mode, const tb_probe_grid* grid,
    float beta, float* out)
{
    if (!grid || !wn_aligned(out, 4) || !grid->count[0] || !grid->count[1] || !grid->count[2]) return hipErrorInvalidValue;
    const uint64_t plane = (uint64_t)grid->count[0] * grid->count[1], cells = plane * grid->count[2];
    if (plane > 0x80000000ull || cells > 0x80000000ull) return hipErrorInvalidValue;
    if (mode == WN_WRITE) return wn_launch(wn_walk_kernel<WN_WRITE, true>, stream, ds, moments, root, (uint32_t)cells, nullptr, *grid, beta, out);
    if (mode == WN_SIGN_CELLS) return wn_launch(wn_walk_kernel<WN_SIGN_CELLS, true>, stream, ds, moments, root, (uint32_t)cells, nullptr, *grid, beta, out);
    return hipErrorInvalidValue;
}
