"""The loop form of the walk steps for scenes in LDS (traverse<..., LDS_STEPS>, pt_device.hpp; docs/experiments/r9.md): both loops leave on
wave-uniform conditions, a lane's own condition only predicates a step.

CPU, compile-only: the listing of pt_variant_matte6.hip under the build's own flags -- the inner-node loop's scalar and total instruction counts at
most the shipped ones, its back edge decided by a scalar compare, and the rest of each walk (the leaf step and the loop control) with no more VALU
instructions than the per-lane loops had.
CPU, a lock-step model: 64 lanes over HostScene.lds_image() through exactly the kernel's control flow -- every lane visits what it visits walking
alone, returns the same hit, and the wave is done within the trips the lanes' own steps add up to.
GPU: the three kernels of the six-wave copy against the oracle, bit for bit, over frame sizes with lanes that have no sample, 1 and 8 bounces and
every park_min that changes which of the loop's branches are taken."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CORNELL, ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))

from test_lds_walk_steps import BASE, DONE, LEAF, SCENES, _boxes, _copy_in, _ray, _rays, _triangle, _walk_image  # noqa: E402

# docs/experiments/r9.md, static table: the inner-node loop as shipped (the per-lane loops before it: 23 scalar ALU of 71 instructions) ...
SALU_SHIPPED = 15
INSTR_SHIPPED = 63
# ... and the VALU instructions of the rest of a walk in the listing of the commit before (scripts/isa_walk_steps.py, "rest of the walk"): the
# bounce ray's walk, the feeler's
REST_VALU_BEFORE = (58, 55)


# ---- the listing -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from tracerboy_amd import build as b
    out = str(tmp_path_factory.mktemp("isa") / "matte6.s")
    src = "kernels/pt_variant_matte6.hip"
    cmd = [b.HIPCC] + b.COMMON + list(b.device_flags(src)) + ["--cuda-device-only", "-S", "-o", out, os.path.join(b.CSRC, src)]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def test_both_walks_of_the_three_kernels_leave_their_inner_loop_on_a_scalar_condition(listing):
    from isa_walk_steps import walk_steps
    kernels = walk_steps(listing)
    tails = sorted(k["name"].rstrip(">").split(", ")[9:] for k in kernels)      # plain, shrinking groups, list-driven
    assert tails == [["false", "false"], ["false", "true"], ["true", "false"]], [k["name"] for k in kernels]
    for k in kernels:
        assert len(k["loops"]) == 2, (k["name"], k["loops"])
        for loop, rest_before in zip(k["loops"], REST_VALU_BEFORE):
            rest = loop["rest"]
            print(k["name"], loop["header"], "SALU", loop["salu"], "instructions", loop["instr"], "back edge", loop["back_edge"],
                  "| rest of the walk", rest and (rest["header"], "VALU", rest["valu"], "LDS", rest["lds"], "SALU", rest["salu"], "instructions", rest["instr"]))
            assert loop["salu"] <= SALU_SHIPPED and loop["instr"] <= INSTR_SHIPPED, (k["name"], loop["header"], loop["salu"], loop["instr"])
            assert loop["back_edge"] and loop["back_edge_scalar"], (k["name"], loop["header"], loop["back_edge"])
            assert rest is not None and rest["depth"] == loop["depth"] - 1
            assert rest["valu"] <= rest_before, (k["name"], rest["header"], rest["valu"])


# ---- the lock-step model -----------------------------------------------------------------------------------------------------------------------
MODEL_SCENES = ["cornell-box/scene.pbrt", "furnace/box.pbrt", "furnace/plane.pbrt"]
PARK_MINS = [1, 2, 8, 64, 4096]
LANES = 64


@pytest.fixture(scope="module", params=MODEL_SCENES)
def scene(request, built):
    from tracerboy_amd import api
    hs = api.HostScene(os.path.join(SCENES, request.param))
    image, info = hs.lds_image()
    nodes, tris, root = hs.layout_b()
    held = _copy_in(image, info, BASE)      # as the kernel holds it
    rays = _rays(dict(nodes=nodes), 320)
    return dict(name=request.param, image=image, info=info, f=held.view(np.float32), u=held.view(np.uint32), rays=rays)


class Lane:
    """one lane's walk state: the ref, the index of the column's top entry, the hit, and what it has visited so far"""

    def __init__(self, scene, o, d, live=True):
        info = scene["info"]
        self.s, self.r = scene, _ray(o, d)
        self.leaf_add = (self.r["copy"] * 3 * 16 + LEAF + BASE + info.off_tris) & 0xffffffff
        self.column = [DONE] + [None] * (info.stack_depth - 1)
        self.sp = 0
        self.ref = (info.root_ref if info.root_ref & LEAF else info.root_ref + BASE) if live else DONE
        self.best, self.visits, self.inner_steps, self.leaf_steps = [1e30, 0.0, 0.0, 0, 0], [], 0, 0

    def copy(self):
        c = Lane.__new__(Lane)
        c.__dict__.update(self.__dict__)
        c.column, c.best, c.visits = list(self.column), list(self.best), list(self.visits)
        return c

    def is_inner(self):
        return not (self.ref & LEAF)

    def at_leaf(self):
        return bool(self.ref & LEAF) and self.ref != DONE

    def pop(self):
        self.ref = self.column[self.sp]
        self.sp -= 1

    def inner_step(self):
        f, u = self.s["f"], self.s["u"]
        at = self.ref - BASE
        assert at % 80 == 0 and 0 <= at and at + 64 <= self.s["info"].off_tris
        self.visits.append(("node", at // 80)); self.inner_steps += 1
        lh, rh, lt, rt = _boxes(f[at // 4:at // 4 + 16], self.r, self.best[0])
        left, right = int(u[at // 4 + 12]), int(u[at // 4 + 13])
        if lh and rh:
            right_first = rt < lt
            self.sp += 1
            self.column[self.sp] = left if right_first else right
            self.ref = right if right_first else left
        elif lh or rh:
            self.ref = right if rh else left
        else:
            self.pop()

    def leaf_step(self):
        f, u, info = self.s["f"], self.s["u"], self.s["info"]
        at = ((self.ref + self.leaf_add) & 0xffffffff) - BASE
        assert info.off_tris <= at and at + 48 <= info.bytes and (at - info.off_tris) % 48 == 0
        self.visits.append(("tri", (at - info.off_tris) // 288)); self.leaf_steps += 1
        rec, words = f[at // 4:at // 4 + 12], u[at // 4:at // 4 + 12]
        _triangle(self.best, [[rec[4 * v + c] for c in range(3)] for v in range(3)], (int(words[3]), int(words[7])), self.r)
        self.pop()

    def walk_alone(self):
        """the lane's own sequence: the loops as a single lane runs them, whatever their form"""
        while self.ref != DONE:
            if self.is_inner():
                self.inner_step()
            else:
                self.leaf_step()
        return self


def run_wave(lanes, park_min):
    """the control flow of traverse<..., LDS_STEPS>, statement for statement: uniform tests on ballots, a lane's own condition as the predicate of a
    step.  Returns (inner trips, leaf trips, passes of the outer loop); a trip is a step the wave issued, for however many lanes."""
    def ballot(pred):
        return sum(1 << i for i, l in enumerate(lanes) if pred(l))
    popc = lambda m: bin(m).count("1")     # noqa: E731
    limit = 1000000
    park_min = max(park_min, 1)
    inner_trips = leaf_trips = passes = 0
    inner = ballot(Lane.is_inner)
    while True:                                         # do {
        passes += 1
        assert passes < limit
        if inner != 0:
            while True:                                 #     do {
                inner_trips += 1
                assert inner_trips < limit
                for l in lanes:
                    if l.is_inner():
                        l.inner_step()
                inner = ballot(Lane.is_inner)
                if not popc(inner) >= park_min:         #     } while (popc(inner) >= parkMin);
                    break
        at_leaf = ballot(Lane.at_leaf)
        busy = inner | at_leaf                          #     before the leaf step
        if at_leaf:
            leaf_trips += 1
            for i, l in enumerate(lanes):
                if (at_leaf >> i) & 1:
                    l.leaf_step()
        inner = ballot(Lane.is_inner)
        if not busy:                                    # } while (busy != 0);
            break
    return inner_trips, leaf_trips, passes


def check_wave(start, park_min):
    """the lanes from the states in `start` in lock step, against each of them walking alone from the same state"""
    alone = [l.copy().walk_alone() for l in start]
    wave = [l.copy() for l in start]
    before_inner, before_leaf = sum(l.inner_steps for l in start), sum(l.leaf_steps for l in start)
    inner_trips, leaf_trips, passes = run_wave(wave, park_min)
    for w, a, s in zip(wave, alone, start):
        assert w.ref == DONE and w.visits == a.visits and w.best == a.best, (park_min, s.r)
        assert w.sp == (-1 if s.ref != DONE else 0)     # the sentinel popped once, by the lanes that walked
    own_inner, own_leaf = sum(l.inner_steps for l in alone) - before_inner, sum(l.leaf_steps for l in alone) - before_leaf
    assert inner_trips <= own_inner and leaf_trips <= own_leaf, (park_min, inner_trips, own_inner, leaf_trips, own_leaf)
    assert passes <= inner_trips + leaf_trips + 1       # every pass but the one that finds the wave idle makes a trip
    return inner_trips, leaf_trips, own_inner, own_leaf


def _hits_root(scene, o, d):
    """the slab test on the box around the root's two children (doubles; which lanes start DONE is the model's choice, not the kernel's rounding)"""
    rec = scene["f"][0:16]
    lo = [min(rec[2 * k] - rec[6 + 2 * k], rec[2 * k + 1] - rec[7 + 2 * k]) for k in range(3)]
    hi = [max(rec[2 * k] + rec[6 + 2 * k], rec[2 * k + 1] + rec[7 + 2 * k]) for k in range(3)]
    t0, t1 = 0.0, 1e30
    for k in range(3):
        if d[k] == 0.0:
            if not lo[k] <= o[k] <= hi[k]:
                return False
            continue
        a, b = (lo[k] - o[k]) / d[k], (hi[k] - o[k]) / d[k]
        t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return t0 <= t1


@pytest.mark.parametrize("park_min", PARK_MINS)
def test_lock_step_lanes_walk_as_they_walk_alone(scene, park_min):
    rays = scene["rays"]
    # anchor: a lane walking alone is the accepted replay of the walk (test_lds_walk_steps.py)
    for o, d in rays[:40]:
        best, visits, _ = _walk_image(scene["image"], scene["info"], _ray(o, d))
        lane = Lane(scene, o, d).walk_alone()
        assert lane.visits == visits and lane.best == best
    totals = np.zeros(4, dtype=np.int64)
    missed = 0
    # whole waves; a ray that misses the root box is a lane that is DONE at entry
    for w in range(0, len(rays), LANES):
        start = [Lane(scene, o, d, live=_hits_root(scene, o, d)) for o, d in rays[w:w + LANES]]
        missed += sum(1 for l in start if l.ref == DONE)
        totals += check_wave(start, park_min)
    live = [Lane(scene, o, d) for o, d in rays if _hits_root(scene, o, d)]
    dead = [Lane(scene, o, d, live=False) for o, d in rays if not _hits_root(scene, o, d)][:LANES]
    assert len(live) >= LANES and len(dead) >= 8, (len(live), len(dead))
    dead = (dead * LANES)[:LANES]
    # every lane DONE at entry: no trip at all
    assert check_wave(dead, park_min)[:2] == (0, 0)
    # one live lane, in the first, the last and a middle lane; a wave of one lane
    for at in (0, 31, 63):
        start = list(dead)
        start[at] = live[at]
        check_wave(start, park_min)
    check_wave([live[1]], park_min)
    # 63 lanes DONE and one at a leaf: lanes stopped where they first stand on a triangle
    at_leaf = []
    for lane in live:
        lane = lane.copy()
        while lane.ref != DONE and not lane.at_leaf():
            lane.inner_step()
        if lane.at_leaf():
            at_leaf.append(lane)
    assert len(at_leaf) >= 16, len(at_leaf)
    for k, lane in enumerate(at_leaf[:16]):
        start = list(dead)
        start[(k * 13) % LANES] = lane
        inner_trips, leaf_trips, _, _ = check_wave(start, park_min)
        assert leaf_trips >= 1
    # a wave of lanes at leaves and lanes still at the root, a wave of lanes at leaves alone
    check_wave((at_leaf[:24] + live[:24] + dead)[:LANES], park_min)
    check_wave(at_leaf[:LANES], park_min)
    print(scene["name"], "park_min", park_min, "inner trips %d for %d lane steps, leaf trips %d for %d; %d lanes DONE at entry" % (totals[0], totals[2], totals[1], totals[3], missed))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
GPU_SCENES = {"cornell-box": CORNELL, "furnace-box": os.path.join(SCENES, "furnace", "box.pbrt")}
_ORACLE = {}
_LOADED = {}    # what the module's context holds: (scene, park_min)


@pytest.fixture(scope="module")
def tb(built):
    """a context of this module's own: park_min is read when a scene is loaded and has no value that means "not set", so the session's context
    is left alone"""
    from tracerboy_amd import api
    ctx = api.TracerBoy(0)
    yield ctx
    ctx.close()
    _LOADED.clear()


def _oracle(tb, name, W, H, F, s):
    """the CPU oracle's surfaces, once per (scene, size, frames, bounces)"""
    import oracle_lib as ol
    key = (name, W, H, F, s.MaxBounces)
    if key not in _ORACLE:
        _ORACLE[key] = ol.render(tb.HostSceneView(), tb.FrameConstants(W, H, 0, s, 0.0), W, H, F, threads=8, jittered=True)
    return _ORACLE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["plain", "shrinking", "list"])
@pytest.mark.parametrize("bounces", [1, 8])
@pytest.mark.parametrize("W,H,F", [(20, 12, 3), (40, 24, 4)])     # partial 8x8 tiles and a partial 16x16 region: lanes with no sample
@pytest.mark.parametrize("park_min", PARK_MINS)
@pytest.mark.parametrize("name", sorted(GPU_SCENES))
def test_uniform_exits_are_bit_equal_to_the_oracle(tb, name, park_min, W, H, F, bounces, kernel):
    from tracerboy_amd import api
    s = api.GetDefaultOutputSettings()
    s.EnableBlueNoise = 0
    s.MaxBounces = bounces
    if _LOADED.get("now") != (name, park_min):
        tb.SetOption("park_min", park_min)      # read by LoadScene
        tb.LoadScene(GPU_SCENES[name])
        _LOADED["now"] = (name, park_min)
    total = F
    try:
        tb.InvalidateHistory()
        if kernel == "list":
            # as in test_lds_walk_steps.py: adaptive sampling tested once per call with a threshold of zero -- the live list is every pixel
            # that is not black after two plain frames, a black pixel keeps those two frames' sums
            total = F + 2
            s.ConvergencePercentage = 0.0
            tb.SetOption("adaptive", 1); tb.SetOption("adaptive_min_frames", 1); tb.SetOption("adaptive_test", 1)
            tb.Render(W, H, 2, s, 0.0)
        tb.Render(W, H, F, s, 0.0, sync=kernel != "plain")
        tb.Sync()
        waves = tb.GetOption("last_copy_waves")
        if waves != 6 and name != "cornell-box":
            pytest.skip("%s does not run the six-wave copy (last_copy_waves %d)" % (name, waves))
        assert waves == 6 and tb.GetOption("last_pipeline") == 0
        if kernel == "list":
            assert tb.GetOption("last_adaptive") == 1
        elif kernel == "shrinking":   # at least two groups per region, the last ones cut small
            assert tb.GetOption("last_plan_guided_groups") == 1 and F >= 2 * tb.GetOption("last_plan_frame_group")
        else:
            assert tb.GetOption("last_plan_guided_groups") == 0 and tb.GetOption("last_adaptive") == 0
        out, jit = tb.ReadAccumulation(jittered=True)
    finally:
        if kernel == "list":
            tb.SetOption("adaptive", 0); tb.SetOption("adaptive_test", 0); tb.SetOption("adaptive_min_frames", 1024)
    ref = _oracle(tb, name, W, H, total, s)
    if kernel == "list":
        from test_adaptive_sampling import skips
        before = _oracle(tb, name, W, H, 2, s)
        black = skips((before["output"], before["jittered"]), 0.0)
        ref = {k: np.where(black[..., None], before[k], ref[k]) for k in ("output", "jittered")}
    diff = int((out.view(np.uint32) != ref["output"].view(np.uint32)).any(axis=-1).sum())
    print(name, park_min, W, H, F, bounces, kernel, "pixels that differ from the oracle:", diff)
    assert np.array_equal(out.view(np.uint32), ref["output"].view(np.uint32)), diff
    assert np.array_equal(jit.view(np.uint32), ref["jittered"].view(np.uint32))
