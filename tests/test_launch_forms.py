"""Which kernel a lock-step launcher runs for a launch, or that it refuses: pt_pick_form (tracerboy_amd/csrc/kernels/pt_copies.h) on the CPU.

tests/forms/forms_driver.cpp prints the picker's answer for every copy and every combination of the fields of a launch's shape.  The expectation
below is the launcher as it stood before the picker existed (pt_variant.inc of commit 0a4a648), written out role by role in the order of its
checks: a base copy, a base copy that carries the pre-pass (surf), the full feature set, an occupancy copy, the copy for scenes in LDS.  A host rule
that asks a copy for a form it refuses (the warm-up of an instanced scene; ADVICE r4: a pipeline chosen where its launcher refused) shows
up here as a difference between the two."""
import collections
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "forms", "_build")

LOCKSTEP, STREAM, LIVE_GROUPS, ADAPTIVE = range(4)
BASE, OCCUPANCY, LDS_GROUPS = range(3)
Shape = collections.namedtuple("Shape", "mode groups list counting sceneLds twoLevel layoutC split overflowFits hits first shrinking")
Copy = collections.namedtuple("Copy", "name set features role waves stash counting streaming prepassInBase nforms")
# per unit: instantiations of pt_persistent, of pt_primary + pt_first (the listings of commit 0a4a648)
KERNELS = {"matte": (9, 0), "env": (9, 0), "sss": (9, 0), "vol": (9, 0), "surf": (11, 2), "full": (11, 0), "matte5": (23, 6), "env5": (23, 6),
           "sss4": (23, 6), "vol4": (23, 6), "matte6": (3, 0)}
EXT = 0x20


def persistent(L, C=0, G=0, HY=0, NC=0, TL=0, PR=0, FI=0, GU=0, AD=0, pre=None):
    """pt_persistent<F, SCENE_LDS, COUNT, GROUPS, HYBRID, NODEC, TWOLEVEL, PRIMARY, FIRST, GUIDED, ADAPTIVE>, and the kernel that runs before it"""
    return (("pt_persistent",) + tuple(int(bool(x)) for x in (L, C, G, HY, NC, TL, PR, FI, GU, AD)), pre)


def stream(L, C):
    return (("pt_stream", int(bool(L)), int(bool(C))), None)


def expected(c, s):
    """the kernels of the launch, or None where the launcher returned hipErrorInvalidValue"""
    only_persistent, only_lds_groups = c.role != BASE, c.role == LDS_GROUPS     # PT_ONLY_PERSISTENT, PT_ONLY_LDS_GROUPS
    ext, L = bool(c.features & EXT), s.sceneLds
    if s.mode == ADAPTIVE:                                                        # pt_launch_adaptive_*: the base copies had one
        if only_persistent: return None
        if not s.list or s.groups or s.hits or s.counting or s.split or s.layoutC: return None
        if not ext and s.twoLevel: return None
        return persistent(L, AD=1)
    guided = s.groups and s.shrinking and L and not s.split and not s.twoLevel and not s.layoutC and not s.hits
    if s.mode == LIVE_GROUPS:                                                     # pipeline == PT_LAUNCH_LIVE_GROUPS
        if not s.groups or not s.list or s.counting or s.hits or s.layoutC or s.shrinking: return None
        if only_lds_groups:
            if not L or s.twoLevel or s.split: return None
            return persistent(1, G=1, AD=1)
        if only_persistent:
            if s.split and not s.overflowFits: return None
            if s.twoLevel: return None if L else persistent(0, G=1, HY=s.split, TL=1, AD=1)
            return persistent(L, G=1, HY=s.split, AD=1)
        if s.split: return None
        if not ext and s.twoLevel: return None
        return persistent(L, G=1, AD=1)
    pipeline = 1 if s.mode == STREAM else 0
    if s.groups and (s.counting or pipeline != 0): return None
    if only_lds_groups:
        if not s.groups or not L or s.counting or s.twoLevel or s.hits or s.layoutC or s.split: return None
        return persistent(1, G=1, GU=guided)

    def pick(C):                                                                  # PT_PICK
        if only_persistent: return None if pipeline != 0 else persistent(L, C)
        return stream(L, C) if pipeline == 1 else persistent(L, C)
    if s.counting: return pick(1) if c.counting else None
    if only_persistent:
        if s.twoLevel:
            if not s.groups or L or s.layoutC: return None
            if s.split and not s.overflowFits: return None
            return persistent(0, G=1, HY=s.split, TL=1)
    elif not ext and s.twoLevel: return None
    if (only_persistent or c.prepassInBase) and not ext:
        if s.hits:
            if not s.groups or L or s.twoLevel: return None
            if s.split and not s.overflowFits: return None
            if not only_persistent and (s.split or s.layoutC): return None
            if s.first:
                if s.layoutC: return None
                return persistent(0, G=1, HY=s.split, PR=1, FI=1, pre=("pt_first", int(s.split)))
            return persistent(0, G=1, HY=s.split, NC=s.layoutC, PR=1, pre=("pt_primary", int(s.split), int(s.layoutC)))
    elif s.hits: return None
    if only_persistent:
        if s.layoutC:
            if not s.groups or L: return None
            if s.split and not s.overflowFits: return None
            return persistent(0, G=1, HY=s.split, NC=1)
    elif s.layoutC: return None
    if only_persistent and s.groups and s.split:
        return persistent(L, G=1, HY=1) if s.overflowFits else None
    if s.split: return None
    if s.groups: return persistent(1, G=1, GU=1) if guided else persistent(L, G=1)
    return pick(0)


@pytest.fixture(scope="module")
def table():
    """-> {copy name: Copy}, {(copy name, Shape): kernels or None}"""
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no g++ / make")
    return picker_table()


_TABLE = []


def picker_table():
    if _TABLE: return _TABLE[0]
    r = subprocess.run(["make", "-C", os.path.join(HERE, "forms"), "OUT=" + BUILD], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    p = subprocess.run([os.path.join(BUILD, "forms_driver")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:] + p.stderr)[-4000:]
    copies, picks = {}, {}
    for line in p.stdout.splitlines():
        w = line.split()
        if w[0] == "copy":
            copies[w[1]] = Copy(w[1], w[2], *[int(x) for x in w[3:]])
        else:
            s, out = Shape(*[int(x) for x in w[2:14]]), [int(x) for x in w[15:]]
            if not out[0]: picks[(w[1], s)] = None
            elif out[1]: picks[(w[1], s)] = stream(out[2], out[3])
            else:
                f = out[2:12]
                pre = {0: None, 1: ("pt_primary", f[3], f[4]), 2: ("pt_first", f[3])}[out[12]]
                picks[(w[1], s)] = (("pt_persistent",) + tuple(f), pre)
    _TABLE.append((copies, picks))
    return _TABLE[0]


def reachable(picks, name):
    """the distinct kernels of a copy, by template: {"pt_persistent": {...}, "pt_stream": {...}, "pt_primary": {...}, "pt_first": {...}}"""
    out = collections.defaultdict(set)
    for (n, _), k in picks.items():
        if n == name and k:
            out[k[0][0]].add(k[0][1:])
            if k[1]: out[k[1][0]].add(k[1][1:])
    return out


def test_the_table_has_the_eleven_copies(table):
    copies, _ = table
    assert sorted(copies) == sorted(KERNELS)
    roles = {n: c.role for n, c in copies.items()}
    assert [n for n in roles if roles[n] == OCCUPANCY] == ["matte5", "env5", "sss4", "vol4"] and [n for n in roles if roles[n] == LDS_GROUPS] == ["matte6"]
    assert [n for n, c in copies.items() if c.prepassInBase] == ["surf"] and [n for n, c in copies.items() if c.counting] == ["full"]
    assert all(c.streaming == (c.role == BASE) for c in copies.values())


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_picker_answers_like_the_launcher_it_replaced(table, name):
    copies, picks = table
    n = 0
    for mode in range(4):
        for bits in itertools.product((0, 1), repeat=11):
            s = Shape(mode, *bits)
            assert picks[(name, s)] == expected(copies[name], s), (name, s)
            n += 1
    assert n == 8192 and sum(1 for k in picks if k[0] == name) == n


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_a_copy_reaches_the_kernels_its_unit_held(table, name):
    copies, picks = table
    r = reachable(picks, name)
    assert (len(r["pt_persistent"]), len(r["pt_primary"]) + len(r["pt_first"])) == KERNELS[name]
    assert len(r["pt_stream"]) == ((4 if copies[name].counting else 2) if copies[name].streaming else 0)
    # the list the unit instantiates from (pt_forms_of) counts launches, pre-pass included: a lock-step kernel behind two pre-passes is one kernel
    launches = {k for (n, _), k in picks.items() if n == name and k}
    assert copies[name].nforms == len(launches)


def mangled(features, kernel):
    name, args = kernel[0], kernel[1:]
    return "_ZN12_GLOBAL__N_1%d%sILj%dE%sEEv" % (len(name), name, features, "".join("Lb%dE" % a for a in args))


def test_every_reachable_kernel_is_in_the_library(table, built):
    from tracerboy_amd import build as b
    copies, picks = table
    lib = open(b.LIB, "rb").read()
    for name, c in copies.items():
        for template, kernels in reachable(picks, name).items():
            for args in kernels:
                assert mangled(c.features, (template,) + args).encode() in lib, (name, template, args)
