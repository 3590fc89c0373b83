"""The list-driven frame-group kernels of the occupancy copies (pt_persistent<..., GROUPS = true, ..., ADAPTIVE = true>) exist in
the built library, and the rule of tests/test_isa_walk_loops.py holds for them: no scratch access inside a walk loop.  Same method -- the listing of
the translation unit, mapped by scripts/isa_spill_map.py; "inside a walk" = loop depth >= 2 by LLVM's own annotation.  Compile-only."""
import os
import sys

import pytest

from conftest import ROOT
from test_isa_walk_loops import _listing

sys.path.insert(0, os.path.join(ROOT, "scripts"))

from test_launch_forms import LIVE_GROUPS, picker_table

UNITS = ["env5", "matte5", "matte6", "sss4", "vol4"]     # the copies that are not a base copy (pt_copies.h)


def list_driven_forms(unit):
    """the forms the unit's launcher can pick for a list-driven frame-group launch (pt_pick_form through tests/forms/forms_driver.cpp):
    (SCENE_LDS, HYBRID, TWOLEVEL)"""
    copies, picks = picker_table()
    assert sorted(n for n, c in copies.items() if c.role != 0) == UNITS
    text = ("false", "true")
    return sorted({(text[k[0][1]], text[k[0][4]], text[k[0][6]]) for (n, s), k in picks.items() if n == unit and k and s.mode == LIVE_GROUPS})


def template_args(name):
    return name[name.index("<") + 1:].rstrip(">").split(", ")


@pytest.mark.parametrize("unit", UNITS)
def test_list_driven_kernels_of_the_occupancy_copies(tmp_path, built, unit):
    from isa_spill_map import spill_map
    from tracerboy_amd import build as b
    text = _listing(tmp_path, unit)
    kernels = {tuple(template_args(k["name"])[1:]): k for k in spill_map(text) if "pt_persistent<" in k["name"]}
    lib = open(b.LIB, "rb").read()
    forms = list_driven_forms(unit)
    assert len(forms) == (1 if unit == "matte6" else 6), forms
    for lds, hybrid, two in forms:
        # <F, SCENE_LDS, COUNT, GROUPS, HYBRID, NODEC, TWOLEVEL, PRIMARY, FIRST, GUIDED, ADAPTIVE>
        args = (lds, "false", "true", hybrid, "false", two, "false", "false", "false", "true")
        assert args in kernels, (unit, args)
        k, plain = kernels[args], kernels[args[:-1] + ("false",)]
        mangled = "pt_persistentILj%sE" % template_args(k["name"])[0].rstrip("u") + "".join("Lb%dE" % (a == "true") for a in args)
        assert ("_ZN12_GLOBAL__N_113" + mangled).encode() in lib, (unit, mangled)
        if lds == "false":
            assert k["walk_loops"] and k["walks"] >= 1, k["name"]           # the mapper found the walks it is asked about
        if two == "false":
            assert k["deep_ld"] == 0 and k["deep_st"] == 0, (k["name"], k["deep_ld"], k["deep_st"])
        else:
            # the two-level walks keep the world ray's slab constants for the way out of an instance (test_isa_walk_loops.py): a handful of
            # reloads, and no store that the plain frame-group kernel of the same form does not have
            assert k["deep_ld"] <= 8 and k["deep_st"] <= plain["deep_st"], (k["name"], k["deep_ld"], k["deep_st"], plain["deep_st"])
        # the list form adds one lookup per drawn sample, outside the walks, so held to the same occupancy (amdgpu_waves_per_eu) it must spill what
        # the plain form spills: that form's static counts plus the ~10 % test_isa_walk_loops.py's budget allows a build (+ 8 for the smallest kernels)
        assert k["scratch_ld"] <= 1.1 * plain["scratch_ld"] + 8 and k["scratch_st"] <= 1.1 * plain["scratch_st"] + 8, (k["name"], k["scratch_ld"],
            plain["scratch_ld"], k["scratch_st"], plain["scratch_st"])
