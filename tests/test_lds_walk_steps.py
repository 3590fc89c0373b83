"""The walk steps of the copy for scenes in LDS (pt_variant_matte6.hip; traverse<..., LDS_STEPS>, pt_device.hpp; docs/experiments/r8.md): child refs of the LDS
image turned into LDS addresses on the way in, a stack bottomed by a sentinel with a running pointer.

CPU, compile-only: the listing of the unit under the build's own flags -- no scratch inside the walks, and the static VALU count of every inner-node
loop pinned below the count of the general step it replaced (35; 20 of them are the two-box test).
CPU, the image through the host export: every ref lands where it must, and a host replay of the sentinel-bottomed walk over the image visits the same
nodes and returns the same hit as the walk over layout B.
GPU: cornell-box through the six-wave copy against the oracle, bit for bit -- the three kernels of the copy, frame sizes that are no multiple of the
16x16 region, 0 / 1 / 8 bounces -- and the other pipelines that read the image against pipeline 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CORNELL, ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
LEAF = 0x80000000
DONE = 0xffffffff

# static VALU instructions of one inner-node step: the general step of the commit before (v_lshl_add addresses, a counted stack) and the LDS steps (docs/experiments/r8.md lists both loops instruction by instruction)
VALU_BEFORE = 35
VALU_PINNED = 29


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from tracerboy_amd import build as b
    out = str(tmp_path_factory.mktemp("isa") / "matte6.s")
    src = "kernels/pt_variant_matte6.hip"
    cmd = [b.HIPCC] + b.COMMON + list(b.device_flags(src)) + ["--cuda-device-only", "-S", "-o", out, os.path.join(b.CSRC, src)]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def test_the_three_kernels_walk_without_scratch_and_with_fewer_valu_instructions(listing):
    from isa_spill_map import spill_map
    from isa_walk_steps import walk_steps
    spills = {k["name"]: k for k in spill_map(listing) if "pt_persistent" in k["name"]}
    kernels = walk_steps(listing)
    # <F, SCENE_LDS, COUNT, GROUPS, HYBRID, NODEC, TWOLEVEL, PRIMARY, FIRST, GUIDED, ADAPTIVE>: plain, shrinking groups, list-driven
    tails = sorted(k["name"].rstrip(">").split(", ")[9:] for k in kernels)
    assert tails == [["false", "false"], ["false", "true"], ["true", "false"]], [k["name"] for k in kernels]
    for k in kernels:
        s = spills[k["name"]]
        assert s["deep_ld"] == 0 and s["deep_st"] == 0, (k["name"], s)
        assert k["deep_scratch"] == 0, k["name"]              # (the mapper above looks for walks that fetch from memory; these fetch from LDS)
        assert len(k["loops"]) == 2, (k["name"], k["loops"])  # the bounce ray's walk and the feeler's
        for loop in k["loops"]:
            print(k["name"], loop["header"], "VALU", loop["valu"], "LDS", loop["lds"], "SALU", loop["salu"], "leaf-bit compares", loop["cmp_leaf"])
            assert loop["depth"] >= 3 and loop["scratch"] == 0
            assert loop["valu"] < VALU_BEFORE and loop["valu"] == VALU_PINNED, (k["name"], loop["header"], loop["valu"])
            # (one compare for the parking ballot and one for the loop's mask: carrying a single value costs more scalar mask bookkeeping than
            # the v_cmp it saves, docs/experiments/r8.md)
            assert loop["lds"] == 6                                  # four node pieces, one push, one pop


# ---- the image ---------------------------------------------------------------------------------------------------------------------------------
IMAGE_SCENES = ["cornell-box/scene.pbrt", "furnace/box.pbrt", "mix-glass/scene.pbrt", "furnace/plane.pbrt"]


@pytest.fixture(scope="module", params=IMAGE_SCENES)
def scene(request, built):
    from tracerboy_amd import api
    hs = api.HostScene(os.path.join(SCENES, request.param))
    image, info = hs.lds_image()
    nodes, tris, root = hs.layout_b()
    return dict(name=request.param, image=image, info=info, nodes=nodes, tris=tris, root=root)


def test_image_refs_land_on_their_records(scene):
    im, info = scene["image"], scene["info"]
    assert info.off_nodes == 0 and info.node_stride == 80 and info.tri_copies == 6 and info.off_tris % 16 == 0 and info.bytes % 16 == 0
    assert info.bytes == len(im) and info.off_tris >= info.num_nodes * 80 and info.off_tris + info.num_tris * 288 <= info.bytes
    # LDS-resident under the default budget (option lds_scene_budget, 40 KB: image + stacks; the shading records of these scenes are a few KB)
    assert info.bytes + info.stack_depth * 1024 <= 36 * 1024
    words = im.view(np.uint32)
    assert info.root_ref == scene["root"] and (info.root_ref & ~LEAF) == 0
    for i in range(info.num_nodes):
        rec = words[i * 20:i * 20 + 16]
        assert np.array_equal(rec[:12], scene["nodes"][i][:12])     # the boxes as in layout B
        for side in (12, 13):
            ref, was = int(rec[side]), int(scene["nodes"][i][side])
            assert (ref & LEAF) == (was & LEAF)
            if ref & LEAF:
                off = ref & ~LEAF       # 16-B units from the first triangle record
                assert off % 18 == 0 and off // 18 == (was & ~LEAF) < info.num_tris
                for copy in range(6):   # what a lane adds: copy * 3 units
                    assert info.off_tris + (off + copy * 3) * 16 + 48 <= info.bytes
            else:
                assert ref % 5 == 0 and ref // 5 == was < info.num_nodes
    for t in range(info.num_tris):      # the six copies: (v[kx], v[ky], v[kz]) of every vertex, the fourth words as they were
        src = scene["tris"][t]
        for kz in range(3):
            for sw in range(2):
                kx = 0 if kz == 2 else kz + 1
                ky = 0 if kx == 2 else kx + 1
                if sw:
                    kx, ky = ky, kx
                at = (info.off_tris + (t * 6 + kz * 2 + sw) * 48) // 4
                got = words[at:at + 12]
                for v in range(3):
                    assert [int(got[4 * v + c]) for c in range(3)] == [int(src[4 * v + k]) for k in (kx, ky, kz)]
                    assert got[4 * v + 3] == src[4 * v + 3]


# A host replay of the walk: traverse()'s order (both children tested when their parent is fetched, the far one parked, the near one next, ties go
# left) with the degenerate-axis constants of ray_assemble.  The two forms share the arithmetic (Python doubles on the fp32 data: what is compared
# is how a step finds its records, not the rounding) and differ in everything the LDS steps changed: where a ref points, how a triangle's copy is
# found, how the stack is kept.
def _ray(o, d):
    a = [abs(x) for x in d]
    z = 0 if (a[0] > a[1] and a[0] > a[2]) else (1 if a[1] > a[2] else 2)
    kx = 0 if z == 2 else z + 1
    ky = 0 if kx == 2 else kx + 1
    if d[z] < 0.0:
        kx, ky = ky, kx
    inv = [2.0 ** 80 if x == 0.0 else 1.0 / x for x in d]
    ainv = [2.0 ** 80 * (1 + 2.0 ** -10) if x == 0.0 else abs(1.0 / x) for x in d]
    return dict(o=o, inv=inv, ainv=ainv, oinv=[o[k] * inv[k] for k in range(3)], k=(kx, ky, z), copy=z * 2 + (1 if d[z] < 0.0 else 0),
                shear=(d[kx] / d[z], d[ky] / d[z], 1.0 / d[z]))


def _boxes(rec, r, closest):
    """(left hit, right hit, left entry, right entry) of a node record's 12 floats"""
    out = []
    for side in (0, 1):
        c = [rec[0 + side], rec[2 + side], rec[4 + side]]
        h = [rec[6 + side], rec[8 + side], rec[10 + side]]
        mid = [c[k] * r["inv"][k] - r["oinv"][k] for k in range(3)]
        tmin = max(max(-h[0] * r["ainv"][0] + mid[0], -h[1] * r["ainv"][1] + mid[1]), -h[2] * r["ainv"][2] + mid[2])
        tmax = min(min(h[0] * r["ainv"][0] + mid[0], h[1] * r["ainv"][1] + mid[1]), h[2] * r["ainv"][2] + mid[2])
        t = max(tmin, 0.0)
        out.append((t < min(tmax, closest), t))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def _triangle(best, verts, meta, r):
    """the watertight test on vertices already in (kx, ky, kz) order; best = [t, u, v, prim, geom]"""
    ox, oy, oz = (r["o"][k] for k in r["k"])
    sx, sy, sz = r["shear"]
    A, B, C = ([v[0] - ox, v[1] - oy, v[2] - oz] for v in verts)
    ax, ay = A[0] - sx * A[2], A[1] - sy * A[2]
    bx, by = B[0] - sx * B[2], B[1] - sy * B[2]
    cx, cy = C[0] - sx * C[2], C[1] - sy * C[2]
    U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
    det = U + V + W
    if (U < 0 or V < 0 or W < 0) and (U > 0 or V > 0 or W > 0):
        return
    if det == 0.0:
        return
    T = W * (sz * C[2]) + (V * (sz * B[2]) + U * (sz * A[2]))
    sT = abs(T) if (T > 0) == (det > 0) else -abs(T)
    if sT < 0 or sT > best[0] * abs(det):
        return
    t = T / det
    if t < best[0] and t > 1e-4:
        best[:] = [t, V / det, W / det, meta[1], meta[0]]


def _walk_layout_b(nodes_f, tris_f, tris_u, root, r):
    best, visits, stack, ref = [1e30, 0.0, 0.0, 0, 0], [], [], root
    while True:
        if ref & LEAF:
            t = ref & ~LEAF
            visits.append(("tri", t))
            rec = tris_f[t]
            _triangle(best, [[rec[4 * v + k] for k in r["k"]] for v in range(3)], (int(tris_u[t][3]), int(tris_u[t][7])), r)
            if not stack:
                return best, visits
            ref = stack.pop()
            continue
        visits.append(("node", ref))
        lh, rh, lt, rt = _boxes(nodes_f[ref], r, best[0])
        left, right = int(nodes_f[ref].view(np.uint32)[12]), int(nodes_f[ref].view(np.uint32)[13])
        if lh and rh:
            right_first = rt < lt
            stack.append(left if right_first else right)
            ref = right if right_first else left
        elif lh or rh:
            ref = right if rh else left
        else:
            if not stack:
                return best, visits
            ref = stack.pop()


def _copy_in(image, info, base):
    """lds_steps_copy_in (pt_device.hpp): the image as the kernel holds it in LDS at address `base` -- an inner ref is the node's address, a leaf ref
    LEAF | the byte offset of the triangle's first copy"""
    out = image.copy()
    u = out.view(np.uint32)
    for i in range(info.num_nodes):
        for side in (12, 13):
            ref = int(u[i * 20 + side])
            u[i * 20 + side] = (((ref << 4) & 0xffffffff) | LEAF) if ref & LEAF else ((ref << 4) + base) & 0xffffffff
    return out


BASE = 9 * 1024 + 112   # where such an image lies: behind the stacks and the kernel's static LDS


def _walk_image(image, info, r):
    """the LDS steps: refs that are addresses, the per-ray leaf term, a column whose entry 0 is DONE and a pointer to its top entry; also the column's
    high-water mark"""
    image = _copy_in(image, info, BASE)
    f, u = image.view(np.float32), image.view(np.uint32)
    best, visits = [1e30, 0.0, 0.0, 0, 0], []
    column = [DONE] + [None] * (info.stack_depth - 1)
    sp, high = 0, 0
    leaf_add = (r["copy"] * 3 * 16 + LEAF + BASE + info.off_tris) & 0xffffffff
    ref = info.root_ref if info.root_ref & LEAF else info.root_ref + BASE
    while ref != DONE:
        if ref & LEAF:
            at = ((ref + leaf_add) & 0xffffffff) - BASE
            assert info.off_tris <= at and at + 48 <= info.bytes and (at - info.off_tris) % 48 == 0
            visits.append(("tri", (at - info.off_tris) // 288))
            rec, words = f[at // 4:at // 4 + 12], u[at // 4:at // 4 + 12]
            _triangle(best, [[rec[4 * v + c] for c in range(3)] for v in range(3)], (int(words[3]), int(words[7])), r)
            ref = column[sp]; sp -= 1
            continue
        ref -= BASE
        assert ref % 80 == 0 and 0 <= ref and ref + 64 <= info.off_tris
        visits.append(("node", ref // 80))
        rec = f[ref // 4:ref // 4 + 16]
        lh, rh, lt, rt = _boxes(rec, r, best[0])
        left, right = int(u[ref // 4 + 12]), int(u[ref // 4 + 13])
        if lh and rh:
            right_first = rt < lt
            sp += 1; high = max(high, sp)
            column[sp] = left if right_first else right     # IndexError past the column: the walk held more than stack_depth - 1 entries
            ref = right if right_first else left
        elif lh or rh:
            ref = right if rh else left
        else:
            ref = column[sp]; sp -= 1
    assert sp == -1     # the sentinel was the last thing popped, once
    return best, visits, high


def _rays(scene, n=1000):
    """random rays through the scene's box, axis-parallel and plane-parallel directions, origins on the faces of node boxes"""
    rng = np.random.default_rng(20260)
    nodes = scene["nodes"].view(np.float32)
    root = nodes[0] if len(nodes) else None
    lo = np.array([min(root[0 + 2 * k] - root[6 + 2 * k], root[1 + 2 * k] - root[7 + 2 * k]) for k in range(3)], dtype=np.float64)
    hi = np.array([max(root[0 + 2 * k] + root[6 + 2 * k], root[1 + 2 * k] + root[7 + 2 * k]) for k in range(3)], dtype=np.float64)
    axes = [np.eye(3)[k] * s for k in range(3) for s in (1.0, -1.0)]
    rays = []
    for i in range(n):
        o = lo + (hi - lo) * (rng.random(3) * 1.4 - 0.2)
        d = rng.normal(size=3)
        kind = i % 5
        if kind == 1:
            d = axes[i % 6].copy()                                # axis-parallel: two degenerate axes
        elif kind == 2:
            d[i % 3] = 0.0                                        # one degenerate axis
        elif kind == 3:                                           # origin on a face of a node's child box (c +- h exactly, as fp32)
            rec = nodes[int(rng.integers(len(nodes)))]
            side, axis, sign = int(rng.integers(2)), int(rng.integers(3)), (1.0 if rng.random() < 0.5 else -1.0)
            c = np.array([rec[0 + side], rec[2 + side], rec[4 + side]], dtype=np.float64)
            h = np.array([rec[6 + side], rec[8 + side], rec[10 + side]], dtype=np.float64)
            o = c + h * (rng.random(3) * 2 - 1)
            o[axis] = float(np.float32(c[axis] + sign * h[axis]))
            if i % 2:
                d = axes[i % 6].copy()
        d = d / np.linalg.norm(d)
        rays.append(([float(np.float32(x)) for x in o], [float(np.float32(x)) for x in d]))
    return rays


def test_sentinel_walk_over_the_image_replays_the_layout_b_walk(scene):
    info = scene["info"]
    nodes_f = scene["nodes"].view(np.float32)
    tris_f, tris_u = scene["tris"].view(np.float32), scene["tris"]
    high_water, hits = 0, 0
    for o, d in _rays(scene):
        r = _ray(o, d)
        best_b, visits_b = _walk_layout_b(nodes_f, tris_f, tris_u, scene["root"], r)
        best_i, visits_i, high = _walk_image(scene["image"], info, r)
        assert visits_i == visits_b, (scene["name"], o, d)
        assert best_i == best_b, (scene["name"], o, d)
        high_water = max(high_water, high)
        hits += best_b[0] < 1e30
    print(scene["name"], "stack high-water", high_water, "of", info.stack_depth, "entries;", hits, "of 1000 rays hit")
    assert high_water <= info.stack_depth - 1
    assert hits >= 100      # the rays do reach the triangles


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def _settings(bounces):
    from tracerboy_amd import api
    s = api.GetDefaultOutputSettings()
    s.EnableBlueNoise = 0
    s.MaxBounces = bounces
    return s


_ORACLE = {}


def _oracle(tb, W, H, F, s):
    """the CPU oracle's surfaces, computed once per (size, frames, bounces)"""
    import oracle_lib as ol
    key = (W, H, F, s.MaxBounces)
    if key not in _ORACLE:
        _ORACLE[key] = ol.render(tb.HostSceneView(), tb.FrameConstants(W, H, 0, s, 0.0), W, H, F, threads=8, jittered=True)
    return _ORACLE[key]


# the three kernels of the copy: a call that waits runs the shrinking-groups kernel, an asynchronous call the plain one, a list-driven call
# (adaptive sampling tested once per call) the list-driven one
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["shrinking", "plain", "list"])
@pytest.mark.parametrize("W,H,F", [(100, 52, 5), (16, 16, 2)])
@pytest.mark.parametrize("bounces", [0, 1, 8])
def test_six_wave_copy_is_bit_equal_to_the_oracle(gpu_tb, kernel, W, H, F, bounces):
    s = _settings(bounces)
    gpu_tb.LoadScene(CORNELL)
    assert gpu_tb.GetOption("scene_in_lds_active") == 1
    total = F
    try:
        gpu_tb.InvalidateHistory()
        if kernel == "list":
            # adaptive sampling tested once per call, with a threshold of zero: the call's live list is every pixel that is not black after the
            # two plain frames before it (a call that starts at or below adaptive_min_frames is plain).  A live pixel's sums are those of a plain
            # render of all the frames, a black pixel keeps its two frames' sums (tb_adaptive_skip, pt_device.hpp).  Without a bounce every pixel
            # is black and the launch finds nothing to do.
            total = F + 2
            s.ConvergencePercentage = 0.0
            gpu_tb.SetOption("adaptive", 1); gpu_tb.SetOption("adaptive_min_frames", 1); gpu_tb.SetOption("adaptive_test", 1)
            gpu_tb.Render(W, H, 2, s, 0.0)
            assert gpu_tb.GetOption("last_adaptive") == 0
        gpu_tb.Render(W, H, F, s, 0.0, sync=kernel != "plain")
        gpu_tb.Sync()
        assert gpu_tb.GetOption("last_copy_waves") == 6 and gpu_tb.GetOption("last_pipeline") == 0
        if kernel == "list":
            assert gpu_tb.GetOption("last_adaptive") == 1 and gpu_tb.GetOption("last_plan_rule_pipeline") == 8   # TB_PLAN_RULE_ADAPTIVE_GROUPS
            live = gpu_tb.LivePixels()
        out, jit = gpu_tb.ReadAccumulation(jittered=True)
    finally:
        if kernel == "list":
            gpu_tb.SetOption("adaptive", 0); gpu_tb.SetOption("adaptive_test", 0); gpu_tb.SetOption("adaptive_min_frames", 1024)
    ref = _oracle(gpu_tb, W, H, total, s)
    if kernel == "list":
        from test_adaptive_sampling import skips
        before = _oracle(gpu_tb, W, H, 2, s)
        black = skips((before["output"], before["jittered"]), 0.0)
        print("live pixels", live, "of", W * H)
        assert live == int((~black).sum()) and (live > 0) == (bounces > 0)
        ref = {k: np.where(black[..., None], before[k], ref[k]) for k in ("output", "jittered")}
    diff = int((out.view(np.uint32) != ref["output"].view(np.uint32)).any(axis=-1).sum())
    print(kernel, W, H, F, bounces, "pixels that differ from the oracle:", diff)
    assert np.array_equal(out.view(np.uint32), ref["output"].view(np.uint32)), diff
    assert np.array_equal(jit.view(np.uint32), ref["jittered"].view(np.uint32))


# the other pipelines copy the same image into LDS and decode its refs in load_node / load_tri
@pytest.mark.gpu
def test_every_pipeline_that_reads_the_image_agrees_with_pipeline_0(gpu_tb):
    W, H, F = 100, 52, 3
    s = _settings(4)
    gpu_tb.LoadScene(CORNELL)
    surfaces = {}
    try:
        for pipeline in (0, 1, 2, 3, 4):
            gpu_tb.SetOption("pipeline", pipeline)
            gpu_tb.InvalidateHistory()
            gpu_tb.Render(W, H, F, s, 0.0)
            assert gpu_tb.GetOption("last_pipeline") == pipeline
            surfaces[pipeline] = gpu_tb.ReadAccumulation(jittered=True)
    finally:
        gpu_tb.SetOption("pipeline", 0)
    assert gpu_tb.GetOption("scene_in_lds_active") == 1
    for pipeline in (1, 2, 3, 4):
        for got, want in zip(surfaces[pipeline], surfaces[0]):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), pipeline
