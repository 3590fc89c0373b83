"""Whether every index the kernels can form into the shading tables is in range: SceneTablesInRange (tracerboy_amd/csrc/host/lds_image.h), the answer
a context needs before it launches the copy whose fetches carry no bounds check (kernels/pt_variant_matte6.hip; docs/experiments/r10.md).

tests/tables/tables_driver.cpp, a host program under ASan + UBSan, runs it on the tables of a two-triangle scene built by hand: sound, and with one
thing broken at a time.  The library's export of the same function is then run on the tables of the committed scenes, whole and broken."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import CORNELL, GOLDEN

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "tables", "_build")

BROKEN = ["geometry_index_past_the_end", "triple_straddles_the_end", "vertex_last_float_past_the_end", "material_index_is_the_count",
          "vertex_index_wraps_in_32_bits", "primitive_index_wraps_in_32_bits"]


def test_the_range_check_on_hand_built_tables_under_sanitizers():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-C", os.path.join(HERE, "tables"), "OUT=" + BUILD], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    p = subprocess.run([os.path.join(BUILD, "tables_driver")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.stdout[-2000:] + p.stderr)[-4000:]
    answers = dict((w[0], int(w[1])) for w in (line.split() for line in p.stdout.splitlines()))
    print(answers)
    assert answers == dict([("sound", 1), ("no_triangles", 1)] + [(name, 0) for name in BROKEN])


def _tables(hs):
    """the tables of a host scene in the form the device holds them: layout-B triangles, hit groups as (MaterialIndex, first vertex float, first
    index, 0), the index buffer, and the two counts"""
    v = hs.view()
    _, tris, _ = hs.layout_b()
    hg = np.array([[v.hitGroups[i].MaterialIndex, v.hitGroups[i].VertexBufferOffset // 4, v.hitGroups[i].IndexBufferOffset // 4, 0]
                   for i in range(v.numHitGroups)], dtype=np.uint32).reshape(-1, 4)
    idx = np.ctypeslib.as_array(v.indexBuffer, shape=(v.numIndices,)).astype(np.uint32)
    return dict(tris=np.ascontiguousarray(tris), hg=hg, idx=idx, vertex_floats=int(v.numVertexFloats), materials=int(v.numMaterials))


def _in_range(t):
    from tracerboy_amd import _ctypes_abi as abi, api
    u32 = C.POINTER(C.c_uint32)
    return api.lib().tb_host_scene_tables_in_range(t["tris"].ctypes.data_as(C.POINTER(abi.TbTriB)), len(t["tris"]), t["hg"].ctypes.data_as(u32), len(t["hg"]),
                                                   t["idx"].ctypes.data_as(u32), len(t["idx"]), t["vertex_floats"], t["materials"])


@pytest.mark.parametrize("scene", ["cornell-box/scene.pbrt", "furnace/box.pbrt"])
def test_the_committed_scenes_are_in_range_and_stop_being_so_when_a_count_shrinks(built, scene):
    from tracerboy_amd import api
    t = _tables(api.HostScene(os.path.join(GOLDEN, "scenes", scene)))
    assert len(t["tris"]) >= 2 and len(t["hg"]) >= 1
    assert _in_range(t) == 1
    # a count one lower than the largest index formed from it needs
    assert _in_range(dict(t, vertex_floats=t["vertex_floats"] - 1)) == 0
    assert _in_range(dict(t, idx=t["idx"][:-1].copy())) == 0
    assert _in_range(dict(t, hg=t["hg"][:-1].copy())) == 0
    assert _in_range(dict(t, materials=int(t["hg"][:, 0].max()))) == 0
    # one index that wraps in 32 bits: 8 * index + first vertex float lands on the vertex it named before
    wrapped = t["idx"].copy()
    wrapped[0] = (int(wrapped[0]) + (1 << 29)) & 0xffffffff
    assert _in_range(dict(t, idx=wrapped)) == 0
    # tables with a count and no pointer are refused, not read
    assert api.lib().tb_host_scene_tables_in_range(None, 1, None, 0, None, 0, 0, 0) < 0
