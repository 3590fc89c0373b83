"""The yardstick and the inputs of tests/test_dynamic_geometry.py.

refit_layout_a restates the fit rule of include/tracerboy_hip.h (tb_commit_geometry) in numpy float32 on a layout-A image (tb_abi.h): every triangle
takes its new vertices, every leaf box is mn = min(v0, v1, v2), mx = max(v0, v1, v2), mn = min(mn, mx - 0.001), c = (mn + mx) * 0.5, h = mx - c, every
inner box comes from its children's STORED c -+ h with the same c, h; child references, metadata and the sorted order stay.  Everything is read from a
TbSceneView, so the same code serves a host scene and a context's own view.

Seeds: displacements use DISPLACE_SEED = 31 (5 % of the extent) and 32 (100 %), normals NORMAL_SEED = 33, ray sets ray_query_cases' own seed 20.  The
CPU tests pin that with those seeds no ray's closest distance differs between the refit tree and a tree built of the moved positions; no seed had to
be replaced."""
import ctypes as C
import os

import numpy as np

import oracle_lib as ol
from conftest import GOLDEN, CORNELL
from tracerboy_amd import _ctypes_abi as abi

LEAF, INDEX_MASK = 0x80000000, 0x00ffffff
DISPLACE_SEED, DISPLACE_SEED_FAR, NORMAL_SEED = 31, 32, 33
PROC_TRIANGLES, PROC_SEED = 10000, 77
DYNAMIC = os.path.join(GOLDEN, "scenes", "dynamic")
INSTANCED = os.path.join(GOLDEN, "scenes", "alpha-card", "instanced.pbrt")
# name -> scene file (None: tb_load_procedural(0, PROC_TRIANGLES, PROC_SEED)); the five one-level scenes
SCENES = {"tri1": os.path.join(DYNAMIC, "tri1.pbrt"), "tri2": os.path.join(DYNAMIC, "tri2.pbrt"), "tri3": os.path.join(DYNAMIC, "tri3.pbrt"),
          "cornell": CORNELL, "proc10k": None}


def bvh_bytes(view):
    return np.ctypeslib.as_array(C.cast(view.bvh, C.POINTER(C.c_uint8)), shape=(view.bvhBytes,)).copy()


def tlas_bytes(view):
    return np.ctypeslib.as_array(C.cast(view.tlas, C.POINTER(C.c_uint8)), shape=(view.tlasBytes,)).copy()


def _sections(image):
    """Views into a layout-A image: nodes (2N - 1, 8) words, primitives (N, 10) words, metadata (N, 3) words."""
    off_boxes, off_prims, off_meta, total = image[:16].view(np.uint32)
    assert off_boxes == 16 and total == image.size and (off_meta - off_prims) % 40 == 0
    n = (off_meta - off_prims) // 40
    assert off_prims == 16 + 32 * (2 * n - 1) and total == off_meta + 12 * n
    words = image.view(np.uint32)
    return words[4:off_prims // 4].reshape(2 * n - 1, 8), words[off_prims // 4:off_meta // 4].reshape(n, 10), words[off_meta // 4:].reshape(n, 3)


def sorted_tri_vertices(view, image=None):
    """(N, 3) vertex numbers of the image's sorted triangles, through the hit-group records and the index buffer as the kernels go."""
    image = bvh_bytes(view) if image is None else image
    _, _, meta = _sections(image)
    groups = np.ctypeslib.as_array(C.cast(view.hitGroups, C.POINTER(C.c_uint32)), shape=(view.numHitGroups, 18))
    indices = np.ctypeslib.as_array(view.indexBuffer, shape=(view.numIndices,))
    g, p = meta[:, 0].astype(np.int64), meta[:, 1].astype(np.int64)
    first_vertex = groups[g, 10].astype(np.int64) // 32        # VertexBufferOffset, bytes of 32-B vertices
    first_index = groups[g, 12].astype(np.int64) // 4          # IndexBufferOffset
    return (indices[first_index[:, None] + 3 * p[:, None] + np.arange(3)].astype(np.int64) + first_vertex[:, None]).astype(np.uint32)


def positions_of(view, image=None):
    """(numVertices, 3) positions as the image's triangles hold them (a vertex no triangle names stays 0)."""
    image = bvh_bytes(view) if image is None else image
    _, prims, _ = _sections(image)
    pos = np.zeros((view.numVertexFloats // 8, 3), np.float32)
    pos[sorted_tri_vertices(view, image).reshape(-1)] = prims[:, 1:].view(np.float32).reshape(-1, 3)
    return pos


def _store(nodes, which, mn, mx):
    c = ((mn + mx) * np.float32(0.5)).astype(np.float32)
    nodes[which, 0:3] = c.view(np.uint32); nodes[which, 4:7] = (mx - c).astype(np.float32).view(np.uint32)


def refit_layout_a(view, new_positions, image=None):
    """The image of `view` (or `image`, which belongs to view's scene) refit to new_positions, (numVertices, 3) float32."""
    out = (bvh_bytes(view) if image is None else image).copy()
    nodes, prims, _ = _sections(out)
    n = prims.shape[0]
    pos = np.ascontiguousarray(new_positions, np.float32)
    v = pos[sorted_tri_vertices(view, out)]                    # (N, 3 vertices, 3)
    prims[:, 1:] = v.reshape(n, 9).view(np.uint32)
    mx = np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 2]); mn = np.minimum(np.minimum(v[:, 0], v[:, 1]), v[:, 2])
    mn = np.minimum(mn, (mx - np.float32(0.001)).astype(np.float32))
    leaf_node = np.arange(n) + (n - 1)
    assert np.array_equal(nodes[leaf_node, 3], (np.arange(n) | LEAF).astype(np.uint32))   # leaf N - 1 + k holds sorted triangle k
    _store(nodes, leaf_node, mn, mx)
    done = np.zeros(2 * n - 1, bool); done[n - 1:] = True
    left, right = (nodes[:n - 1, 3] & INDEX_MASK).astype(np.int64), nodes[:n - 1, 7].astype(np.int64)
    while not done[:n - 1].all():                               # one level per pass: each feeds the next
        ready = np.flatnonzero(~done[:n - 1] & done[left] & done[right])
        assert len(ready)
        f = nodes.view(np.float32)
        l, r = left[ready], right[ready]
        mn = np.minimum(f[l, 0:3] - f[l, 4:7], f[r, 0:3] - f[r, 4:7]); mx = np.maximum(f[l, 0:3] + f[l, 4:7], f[r, 0:3] + f[r, 4:7])
        _store(nodes, ready, mn.astype(np.float32), mx.astype(np.float32))
        done[ready] = True
    return out


def with_bvh(view, image):
    """A copy of the view whose layout-A image is `image` (which the caller keeps alive)."""
    v = abi.TbSceneView.from_buffer_copy(view)
    v.bvh = image.ctypes.data; v.bvhBytes = image.size
    return v


def extent(positions):
    return float(np.max(positions.max(axis=0) - positions.min(axis=0)))


def displaced(positions, fraction, seed, keep=None):
    """Every vertex moved by a seeded offset, uniform in +-fraction x the largest side of the bounds per axis; the vertices `keep` (a boolean mask)
    stay."""
    rng = np.random.default_rng(seed)
    out = (positions + rng.uniform(-1, 1, positions.shape) * fraction * extent(positions)).astype(np.float32)
    if keep is not None:
        out[keep] = positions[keep]
    return out


def emissive_vertices(view):
    """Boolean mask over the vertices: those of a geometry whose material carries TB_MAT_LIGHT (0x10)."""
    groups = np.ctypeslib.as_array(C.cast(view.hitGroups, C.POINTER(C.c_uint32)), shape=(view.numHitGroups, 18))
    nv = view.numVertexFloats // 8
    firsts = sorted(set(int(o) // 32 for o in groups[:, 10])) + [nv]
    mask = np.zeros(nv, bool)
    for g in range(view.numHitGroups):
        if view.materials[int(groups[g, 8])].Flags & 0x10:
            first = int(groups[g, 10]) // 32
            mask[first:firsts[firsts.index(first) + 1]] = True
    return mask


def tri_dict(view, image, positions):
    """What oracle_lib.validate_bvh / build_lbvh take: the triangles in the image's sorted order."""
    _, _, meta = _sections(image)
    return dict(positions=positions, tri_vertex_index=sorted_tri_vertices(view, image), tri_geometry=meta[:, 0].copy(), tri_primitive=meta[:, 1].copy(),
                tri_flags=meta[:, 2].copy())


def bounds_of(view, image):
    _, prims, _ = _sections(image)
    v = prims[:, 1:].view(np.float32).reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)
