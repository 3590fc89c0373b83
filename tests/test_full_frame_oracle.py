"""-m gpu: whole frames at the bench's sizes against the CPU oracle, bit for bit, in the call shapes the bench runs.

The strip tests (test_gpu_parity.py, test_vw_van.py) hold 1 % of a 4K frame to the oracle and the rest HIP against HIP.  Here every workload of
bench.WORKLOADS -- its tree, size, depth, settings and call shapes imported from bench.py, not restated -- is rendered whole and compared with
one oracle render of the whole frame:
  sync1   the first synchronous call after the load (no region costs counted yet);
  sync2   the same call again: launches of the feature sets with interior walks now hand out the regions the first call counted first;
  async   bench.settle_overlap, then 3 x (InvalidateHistory; Render(sync=False)) and Sync -- the launch the bench times (the copy without
          guided groups, frame groups of up to 16 on memory scenes, the two side streams);
  rank r  (legs with a scale_ counterpart) rank 3 / 7 of 8 with the leg's tile size: its own pixels, two synchronous calls and the
          asynchronous shape, the second call on the reordered item list.
F = min(spp, 16) frames; legs with more samples than that render their full count in the asynchronous shape and are compared on three
8-row strips.  Then the frame-size limits: 16384 pixels a side (region coordinates at their 10-bit top) rendered and compared whole,
16385 refused.  Each test owns a context of its own, so nothing it settles (overlap trial, region costs) reaches another test.  Every
comparison's plan fields are in its assertion message and in the line the test prints (`pytest -s`)."""
import contextlib
import copy
import json
import time
import types

import numpy as np
import pytest

import bench
import oracle_lib as ol
from conftest import CORNELL
from test_gpu_parity import bits, load_bench_workload

pytestmark = pytest.mark.gpu
PLAN_FIELDS = ("last_variant", "last_plan_frame_group", "last_plan_guided_groups", "last_plan_costly_first", "last_overlap", "last_primary_prepass")
COSTLY_FIRST_LIMIT = 3 << 24       # launch_plan.h: costly regions first for calls below 3 x 2^24 own samples only
RANKS, WORLD = (3, 7), 8


@contextlib.contextmanager
def fresh_context():
    from tracerboy_amd import api
    tb = api.TracerBoy(0)
    try:
        yield tb
    finally:
        tb.close()


def bench_settings(depth):
    """bench.Bench.settings exactly (it reads nothing of the bench object but its api module)"""
    from tracerboy_amd import api
    return bench.Bench.settings(types.SimpleNamespace(api=api), depth)


def plan(tb):
    return {k: tb.GetOption(k) for k in PLAN_FIELDS}


def owned_mask(W, H, rank, world, tile):
    """pixels of `rank` under the row-major tile deal (tile t belongs to rank t % world; tracerboy_amd/tiles.py)"""
    tx, ty = -(-W // tile), -(-H // tile)
    m = np.zeros((H, W), bool)
    for t in range(rank, tx * ty, world):
        x0, y0 = (t % tx) * tile, (t // tx) * tile
        m[y0:y0 + tile, x0:x0 + tile] = True
    return m


def compare(got, ref, what, pl, mask=None, rows=None):
    """Every bit of (output, jittered) against the oracle's, on the pixels of `mask` / the rows `rows` (all by default).  Returns the
    number of pixels compared."""
    n = 0
    for name, g, r in (("output", got[0], ref[0]), ("jittered", got[1], ref[1])):
        if rows is not None:
            g, r = g[rows[0]:rows[1]], r[rows[0]:rows[1]]
        diff = (bits(g) != bits(r)).any(axis=-1)
        if mask is not None:
            diff &= mask
        n = int(mask.sum()) if mask is not None else diff.size
        bad = int(diff.sum())
        if bad:
            ys, xs = np.nonzero(diff)
            y0 = rows[0] if rows is not None else 0
            raise AssertionError("%s: %s surface differs from the oracle in %d of %d pixels (first at x=%d y=%d, rows %d..%d); plan %s"
                                 % (what, name, bad, n, xs[0], ys[0] + y0, ys.min() + y0, ys.max() + y0, pl))
    return n


def render_sync(tb, W, H, F, s):
    tb.InvalidateHistory()
    tb.Render(W, H, F, s, 0.0)
    pl = plan(tb)
    # a call that waits gets the GUIDED copy (groups that shrink at the launch's end) where the scene is in LDS and the frames make two
    # groups or more; no other call does
    guided = int(bool(tb.GetOption("scene_in_lds_active")) and F >= 2 * pl["last_plan_frame_group"])
    assert pl["last_plan_guided_groups"] == guided, "synchronous %dx%d x %d: %s" % (W, H, F, pl)
    return tb.ReadAccumulation(jittered=True), pl


def render_async(tb, W, H, F, s):
    """the bench's timed shape: the overlap trial settled, then back-to-back asynchronous calls, waited for once"""
    bench.settle_overlap(tb, W, H, F, s)
    for _ in range(3):
        tb.InvalidateHistory()
        tb.Render(W, H, F, s, 0.0, sync=False)
    tb.Sync()
    return tb.ReadAccumulation(jittered=True), plan(tb)


def oracle_frame(tb, W, H, F, s, y0=0, y1=None):
    t0 = time.perf_counter()
    r = ol.render(tb.HostSceneView(), tb.FrameConstants(W, H, 0, s, 0.0), W, H, F, y0=y0, y1=y1, threads=bench.oracle_threads(), jittered=True)
    return (r["output"], r["jittered"]), time.perf_counter() - t0


def report(name, rec):
    print("full-frame %s %s" % (name, json.dumps(rec, sort_keys=True)))


@pytest.mark.parametrize("key", list(bench.WORKLOADS))
def test_bench_workload_whole_frame_is_the_oracle(built, key):
    w0 = bench.WORKLOADS[key]
    W, H, spp = w0["W"], w0["H"], w0["spp"]
    F = min(spp, 16)
    s = bench_settings(w0["depth"])
    rec = {"W": W, "H": H, "F": F, "oracle_threads": bench.oracle_threads(), "shapes": []}
    t_start = time.perf_counter()
    with fresh_context() as tb:
        w = load_bench_workload(tb, key)
        assert w is w0
        ref, rec["oracle_s"] = oracle_frame(tb, W, H, F, s)
        over_limit = W * H * F >= COSTLY_FIRST_LIMIT

        def check(shape, got, pl, mask=None, rows=None):
            what = "%s %s (%dx%d, %d frames)" % (key, shape, W, H, F)
            n = compare(got, ref, what, pl, mask=mask, rows=rows)
            rec["shapes"].append({"shape": shape, "plan": pl, "pixels": n})

        for shape in ("sync1", "sync2"):
            got, pl = render_sync(tb, W, H, F, s)
            check(shape, got, pl)
            del got
            if over_limit:                  # the whole 4K frame at 8 spp: above the costly-first limit, whatever the feature set
                assert pl["last_plan_costly_first"] == 0, "%s %s: %s" % (key, shape, pl)
        got, pl = render_async(tb, W, H, F, s)
        check("async", got, pl)
        del got
        assert pl["last_plan_guided_groups"] == 0, "%s async: %s" % (key, pl)
        if over_limit:
            assert pl["last_plan_costly_first"] == 0, "%s async: %s" % (key, pl)

        if key in bench.SCALE_LEGS:
            tile = w.get("tile", bench.TILE)
            rec["tile"] = tile
            try:
                tb.SetOption("overlap_launches", 2)         # as bench.scale_leg runs a rank
                for rank in RANKS:
                    tb.SetTileAssignment(rank, WORLD, tile, tile)
                    mask = owned_mask(W, H, rank, WORLD, tile)
                    for shape in ("sync1", "sync2"):
                        got, pl = render_sync(tb, W, H, F, s)
                        check("rank%d %s" % (rank, shape), got, pl, mask=mask)
                        del got
                    assert pl["last_plan_costly_first"] == 1, "%s rank %d sync2 did not run on the reordered items: %s" % (key, rank, pl)
                    got, pl = render_async(tb, W, H, F, s)
                    check("rank%d async" % rank, got, pl, mask=mask)
                    del got
                    assert pl["last_plan_guided_groups"] == 0, "%s rank %d async: %s" % (key, rank, pl)
            finally:
                tb.SetTileAssignment(0, 1, 64, 64); tb.SetOption("overlap_launches", 1)
        del ref

        if F < spp:
            # the leg's own sample count in the timed shape, on three strips: the top rows, the last region row (half outside the frame
            # at 1080 = 67 x 16 + 8) and rows across a 64-row tile boundary
            got, pl = render_async(tb, W, H, spp, s)
            assert pl["last_plan_guided_groups"] == 0, "%s async at %d spp: %s" % (key, spp, pl)
            mid = (H // 2) // 64 * 64
            for y0 in (0, H - 8, mid - 4):
                strip, _ = oracle_frame(tb, W, H, spp, s, y0=y0, y1=y0 + 8)
                n = compare(got, strip, "%s async at %d spp, rows %d..%d" % (key, spp, y0, y0 + 7), pl, rows=(y0, y0 + 8))
                rec["shapes"].append({"shape": "async %dspp rows %d-%d" % (spp, y0, y0 + 7), "plan": pl, "pixels": n})
            del got
    rec["wall_s"] = round(time.perf_counter() - t_start, 1)
    rec["oracle_s"] = round(rec["oracle_s"], 1)
    report(key, rec)


SIZE_SCENES = {"glass": lambda tb: tb.LoadProcedural(1, 20000, 5),      # fetched from memory, interior walks: costly regions first applies
               "cornell": lambda tb: tb.LoadScene(CORNELL)}              # scene in LDS


@pytest.mark.parametrize("size", [(16384, 16), (16, 16384), (16384, 40)], ids=lambda wh: "%dx%d" % wh)
@pytest.mark.parametrize("scene", list(SIZE_SCENES))
def test_largest_frames_whole_frame_is_the_oracle(settings, scene, size):
    """The largest frames tb_render accepts (16384 a side): a region's 10-bit coordinates (slot entries, regionCost[ry << 10 | rx]) reach
    1023.  Whole frame, every bit: two synchronous calls, the asynchronous shape, and for the glass scene rank 7 of 8 on 64-px tiles,
    whose tiles include the last one of the row / column."""
    W, H = size
    F = 6
    s = copy.copy(settings); s.MaxBounces = 6
    rec = {"W": W, "H": H, "F": F, "shapes": []}
    with fresh_context() as tb:
        SIZE_SCENES[scene](tb)
        ref, rec["oracle_s"] = oracle_frame(tb, W, H, F, s)
        costly = scene == "glass"
        for shape in ("sync1", "sync2"):
            got, pl = render_sync(tb, W, H, F, s)
            rec["shapes"].append({"shape": shape, "plan": pl, "pixels": compare(got, ref, "%s %dx%d %s" % (scene, W, H, shape), pl)})
            assert pl["last_plan_frame_group"] >= 1 and pl["last_plan_costly_first"] == int(costly), pl
        got, pl = render_async(tb, W, H, F, s)
        rec["shapes"].append({"shape": "async", "plan": pl, "pixels": compare(got, ref, "%s %dx%d async" % (scene, W, H), pl)})
        assert pl["last_plan_guided_groups"] == 0, pl
        if costly:
            try:
                tb.SetTileAssignment(7, 8, 64, 64)
                mask = owned_mask(W, H, 7, 8, 64)
                assert mask[-1, -1]
                for shape in ("sync1", "sync2"):
                    got, pl = render_sync(tb, W, H, F, s)
                    rec["shapes"].append({"shape": "rank7 " + shape, "plan": pl,
                                          "pixels": compare(got, ref, "%s %dx%d rank 7 %s" % (scene, W, H, shape), pl, mask=mask)})
                assert pl["last_plan_costly_first"] == 1, pl
                got, pl = render_async(tb, W, H, F, s)
                rec["shapes"].append({"shape": "rank7 async", "plan": pl,
                                      "pixels": compare(got, ref, "%s %dx%d rank 7 async" % (scene, W, H), pl, mask=mask)})
            finally:
                tb.SetTileAssignment(0, 1, 64, 64)
    rec["oracle_s"] = round(rec["oracle_s"], 2)
    report("%s_%dx%d" % (scene, W, H), rec)


@pytest.mark.parametrize("scene", list(SIZE_SCENES))
def test_frames_beyond_16384_are_refused(settings, scene):
    """16385 pixels a side is refused with TB_E_INVALID (nothing launched), and the context renders the oracle's picture afterwards."""
    from tracerboy_amd import api
    s = copy.copy(settings); s.MaxBounces = 6
    with fresh_context() as tb:
        SIZE_SCENES[scene](tb)
        for W, H in ((16385, 8), (8, 16385)):
            with pytest.raises(api.TracerBoyError) as e:
                tb.Render(W, H, 2, s, 0.0)
            assert e.value.code == -1, (W, H, e.value)           # TB_E_INVALID
            with pytest.raises(api.TracerBoyError):
                tb.Render(W, H, 2, s, 0.0, sync=False)
        W, H, F = 200, 120, 6
        got, pl = render_sync(tb, W, H, F, s)
        ref, _ = oracle_frame(tb, W, H, F, s)
        compare(got, ref, "%s %dx%d after refused sizes" % (scene, W, H), pl)
