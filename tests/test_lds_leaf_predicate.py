"""The leaf step of the walk for scenes in LDS with one predicate in front of the division (tri_test_lds, pt_device.hpp), and the six-wave copy's
unguarded fetches of the shading tables (PT_TABLES_CHECKED, pt_variant_matte6.hip; docs/experiments/r10.md).

CPU, compile-only: the listing of pt_variant_matte6.hip under the build's own flags -- the rest of each walk (the leaf step and the loop control) with
no more instructions and no more scalar ALU instructions than the shipped tree compiles to, no scratch access inside the walks, and no more scratch
per kernel than the commit before had.
GPU: cornell-box through the six-wave copy against the oracle, bit for bit, at frame sizes with lanes that have no sample, and every park_min that
changes which lanes stand at a leaf together; and a call whose LightCount is above the scene's light count, which must run the five-wave copy with
its guards and still match the oracle."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CORNELL, ROOT

sys.path.insert(0, os.path.join(ROOT, "scripts"))

# docs/experiments/r10.md, static table: the rest of a walk as shipped, the bounce ray's walk / the feeler's (the commit before: 108 / 103
# instructions, 29 / 27 of them scalar ALU) ...
REST_INSTR_SHIPPED = (88, 84)
REST_SALU_SHIPPED = (16, 14)
# ... and the scratch of each of the unit's kernels in the commit before
SCRATCH_BYTES_BEFORE = 80


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from tracerboy_amd import build as b
    out = str(tmp_path_factory.mktemp("isa") / "matte6.s")
    src = "kernels/pt_variant_matte6.hip"
    cmd = [b.HIPCC] + b.COMMON + list(b.device_flags(src)) + ["--cuda-device-only", "-S", "-o", out, os.path.join(b.CSRC, src)]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def test_the_rest_of_both_walks_is_no_longer_than_shipped(listing):
    from isa_walk_steps import walk_steps
    kernels = walk_steps(listing)
    tails = sorted(k["name"].rstrip(">").split(", ")[9:] for k in kernels)      # plain, shrinking groups, list-driven
    assert tails == [["false", "false"], ["false", "true"], ["true", "false"]], [k["name"] for k in kernels]
    for k in kernels:
        assert len(k["loops"]) == 2, (k["name"], k["loops"])
        print(k["name"], "scratch accesses at loop depth >= 2:", k["deep_scratch"])
        assert k["deep_scratch"] == 0, (k["name"], k["deep_scratch"])
        for loop, instr, salu in zip(k["loops"], REST_INSTR_SHIPPED, REST_SALU_SHIPPED):
            rest = loop["rest"]
            assert rest is not None and rest["depth"] == loop["depth"] - 1
            print(k["name"], "rest of the walk", rest["header"], "instructions", rest["instr"], "VALU", rest["valu"], "LDS", rest["lds"], "SALU", rest["salu"])
            assert rest["instr"] <= instr and rest["salu"] <= salu, (k["name"], rest["header"], rest["instr"], rest["salu"])


def test_no_kernel_of_the_unit_has_more_scratch_than_before(listing):
    scratch = [int(x) for x in re.findall(r"^\s*\.private_segment_fixed_size:\s*(\d+)", listing, re.M)]
    print("scratch bytes per kernel:", scratch)
    assert len(scratch) == 3 and max(scratch) <= SCRATCH_BYTES_BEFORE, scratch


def test_the_unit_fetches_the_tables_unguarded_and_no_other_does():
    """the define sits in the one unit: every other unit compiles the guarded fetches, textually what they were"""
    kernels = os.path.join(ROOT, "tracerboy_amd", "csrc", "kernels")
    defining = sorted(f for f in os.listdir(kernels) if re.search(r"^\s*#\s*define\s+PT_TABLES_CHECKED\b", open(os.path.join(kernels, f)).read(), re.M))
    assert defining == ["pt_variant_matte6.hip"], defining


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}
_LOADED = {}    # what the module's context holds: park_min
CASES = [(40, 24, 4), (64, 48, 8)]      # A: no multiple of 16, lanes draw samples outside the frame; B: whole regions, eight frames
PARK_MINS = [1, 2, 64]
BOUNCES = 8


@pytest.fixture(scope="module")
def tb(built):
    """a context of this module's own: park_min is read when a scene is loaded and has no value that means "not set", so the session's context
    is left alone"""
    from tracerboy_amd import api
    ctx = api.TracerBoy(0)
    yield ctx
    ctx.close()
    _LOADED.clear()


def _settings():
    from tracerboy_amd import api
    s = api.GetDefaultOutputSettings()
    s.EnableBlueNoise = 0
    s.MaxBounces = BOUNCES
    return s


def _load(tb, park_min):
    if _LOADED.get("now") != park_min:
        tb.SetOption("park_min", park_min)      # read by LoadScene
        tb.LoadScene(CORNELL)
        _LOADED["now"] = park_min


def _oracle(tb, W, H, F, s, light_count=None):
    """the CPU oracle's surfaces on the context's host scene, once per (size, frames, light count)"""
    import oracle_lib as ol
    key = (W, H, F, light_count)
    if key not in _ORACLE:
        pf = tb.FrameConstants(W, H, 0, s, 0.0)
        if light_count is not None:
            pf.LightCount = light_count
        _ORACLE[key] = ol.render(tb.HostSceneView(), pf, W, H, F, threads=8, jittered=True)
    return _ORACLE[key]


def _compare(out, jit, ref, what):
    diff = int((out.view(np.uint32) != ref["output"].view(np.uint32)).any(axis=-1).sum())
    print(*what, "pixels that differ from the oracle:", diff)
    assert np.array_equal(out.view(np.uint32), ref["output"].view(np.uint32)), diff
    assert np.array_equal(jit.view(np.uint32), ref["jittered"].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["plain", "shrinking"])
@pytest.mark.parametrize("W,H,F", CASES)
@pytest.mark.parametrize("park_min", PARK_MINS)
def test_six_wave_copy_is_bit_equal_to_the_oracle(tb, park_min, W, H, F, kernel):
    s = _settings()
    _load(tb, park_min)
    tb.InvalidateHistory()
    tb.Render(W, H, F, s, 0.0, sync=kernel != "plain")
    tb.Sync()
    assert tb.GetOption("last_copy_waves") == 6 and tb.GetOption("last_pipeline") == 0
    if kernel == "shrinking":     # at least two groups per region, the last ones cut small
        assert tb.GetOption("last_plan_guided_groups") == 1 and F >= 2 * tb.GetOption("last_plan_frame_group")
    else:
        assert tb.GetOption("last_plan_guided_groups") == 0 and tb.GetOption("last_adaptive") == 0
    out, jit = tb.ReadAccumulation(jittered=True)
    _compare(out, jit, _oracle(tb, W, H, F, s), (park_min, W, H, F, kernel))


@pytest.mark.gpu
def test_a_light_count_above_the_table_runs_the_guarded_copy(tb):
    """(uint32_t)(rnd * LightCount) can then name a light past the table: the call keeps the five-wave copy, whose fetch gives zeros there, like the
    oracle's"""
    W, H, F = CASES[0]
    s = _settings()
    _load(tb, 2)
    lights = int(tb.HostSceneView().numLights)
    assert lights >= 1
    try:
        tb.SetOption("debug_light_count", lights + 1)
        tb.Render(W, H, F, s, 0.0)
        assert tb.GetOption("last_copy_waves") == 5 and tb.GetOption("last_pipeline") == 0
        out, jit = tb.ReadAccumulation(jittered=True)
    finally:
        tb.SetOption("debug_light_count", 0)
    ref = _oracle(tb, W, H, F, s, light_count=lights + 1)
    _compare(out, jit, ref, ("LightCount", lights + 1, W, H, F))
    # the extra light is seen: some path drew the index past the table and found a light of zeros
    plain = _oracle(tb, W, H, F, s)
    assert not np.array_equal(ref["output"].view(np.uint32), plain["output"].view(np.uint32))
    # and the same call without the option is the six-wave copy's again
    tb.Render(W, H, F, s, 0.0)
    assert tb.GetOption("last_copy_waves") == 6
    out, jit = tb.ReadAccumulation(jittered=True)
    _compare(out, jit, plain, ("LightCount", lights, W, H, F))
