#!/usr/bin/env python3
"""Static cost of one inner-node step of the walks in an assembly listing: for every kernel, the innermost loops (by LLVM's own loop
annotation of the listing) that hold the nine v_pk_fma_f32 of the two-box test, with their VALU, LDS and scalar instruction counts; how each
of them decides its back edge; and the same counts for the rest of its walk -- the blocks of the loop around it that are not its own: the leaf
step and the loop control.
   hipcc ... -S -o k.s pt_variant_matte6.hip;  python scripts/isa_walk_steps.py k.s [substring of the demangled kernel name]
tests/test_lds_walk_steps.py and tests/test_lds_walk_uniform_exits.py pin the counts of the LDS-resident frame-group kernels
(docs/experiments/r8.md, r9.md)."""
import re, subprocess, sys


def walk_steps(text, want=""):
    """[{name, deep_scratch, loops: [{header, depth, valu, lds, salu, cmp_leaf, scratch, instr, ins, back_edge, back_edge_scalar, rest}, ...]}]: the
    inner-node loops of every pt_persistent kernel whose demangled name contains `want`, in listing order (slot 1's walk -- the bounce ray -- comes
    before the feeler's).  back_edge: the conditional branches that decide the ways back to the loop's header; back_edge_scalar: each of them is an
    s_cbranch_scc*.  rest: {header, depth, valu, lds, salu, instr, ins} of the blocks whose
    innermost loop is the loop around this one (None where there is none)"""
    out = []
    for m in re.finditer(r"^(_ZN\S*pt_persistent\S*):.*$", text, re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\(anonymous namespace\)::", "", name); name = re.sub(r"\(.*", "", name).replace("void ", "")
        if want not in name: continue
        body = text[m.start():text.index(".end_amdhsa_kernel", m.start())]
        loops, order, cur, label = {}, [], None, None
        blocks = []     # every labelled block in listing order: {label, loop: header of its innermost loop, ins}

        def enter(header, depth):
            if header not in order: order.append(header)
            return loops.setdefault(header, {"header": header, "depth": depth, "ins": [], "parent": None})
        for line in body.split("\n"):
            if re.match(r"^\.LBB\d+_\d+:", line) or re.match(r"^; %bb\.\d+:", line):
                hdr = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", line)
                lab = re.match(r"^\.L(BB\d+_\d+):", line)
                label = lab.group(1) if lab else None
                blocks.append({"label": label, "loop": None, "ins": []})
                cur = enter(hdr.group(1), int(hdr.group(2))) if hdr else None
                own = re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", line)
                if own and label: cur = enter(label, int(own.group(1)))
                par = re.search(r"Parent Loop (BB\d+_\d+) Depth=\d+", line)
                parent = par.group(1) if par else None
            elif label and line.lstrip().startswith(";") and re.search(r"Parent Loop (BB\d+_\d+) Depth=\d+", line):
                parent = re.search(r"Parent Loop (BB\d+_\d+)", line).group(1)     # (outermost first: the last one named is the loop around)
            elif label and line.lstrip().startswith(";") and re.search(r"=>\s*This (?:Inner )?Loop Header: Depth=(\d+)", line):
                # a loop's header block: the label line names its parents, a comment line below it the loop itself
                cur = enter(label, int(re.search(r"Depth=(\d+)", line.split("=>")[1]).group(1)))
                cur["parent"] = parent
            elif blocks:
                s = line.strip()
                if s and re.match(r"^[a-z]", s):
                    blocks[-1]["ins"].append(s)
                    if cur is not None: cur["ins"].append(s); blocks[-1]["loop"] = cur["header"]
        rows = []

        def counts(ins):
            return {"instr": len(ins), "valu": sum(1 for i in ins if i.startswith("v_")), "lds": sum(1 for i in ins if i.startswith("ds_")),
                    "salu": sum(1 for i in ins if i.startswith("s_") and not re.match(r"s_(waitcnt|nop|c?branch)", i))}
        for h in order:
            ins = loops[h]["ins"]
            if sum(1 for i in ins if i.startswith("v_pk_fma_f32")) != 9: continue
            # what decides each way back to the header: a conditional branch to it; an s_branch to it, or a fall into it from the block listed in
            # front of it, behind a conditional branch out of the loop ("none": that block is reached and left unconditionally)
            back = []
            for k, b in enumerate(blocks):
                if b["loop"] != h: continue
                last = b["ins"][-1] if b["ins"] else ""
                before = b["ins"][-2] if len(b["ins"]) > 1 else ""
                falls = k + 1 < len(blocks) and blocks[k + 1]["label"] == h and not last.startswith("s_branch")
                for i in b["ins"][:-1] + ([] if falls else [last]):
                    if re.match(r"s_cbranch\w*\s+\.L%s$" % h, i): back.append(i.split()[0])
                if re.match(r"s_branch\s+\.L%s$" % h, last): back.append(before.split()[0] if before.startswith("s_cbranch") else "none")
                if falls: back.append(last.split()[0] if last.startswith("s_cbranch") else "none")
            scalar = bool(back) and all(i.startswith("s_cbranch_scc") for i in back)
            around = loops.get(loops[h]["parent"])
            rest = dict(counts(around["ins"]), header=around["header"], depth=around["depth"], ins=around["ins"]) if around else None
            rows.append({"header": h, "depth": loops[h]["depth"], "back_edge": back, "back_edge_scalar": scalar, "rest": rest,
                         **counts(ins),
                         # compares of a child ref with -1: "is it an inner node" (leaf refs and DONE have the sign bit)
                         "cmp_leaf": sum(1 for i in ins if re.match(r"v_cmp\w*_(lt|gt|le|ge)_i32\w*\s.*(-1|, 0)\b", i)),
                         "scratch": sum(1 for i in ins if i.startswith("scratch_")), "ins": ins})
        # scratch accesses inside any loop nested in the path loop (depth >= 2: the walks, the sample-number loop)
        out.append({"name": name, "loops": rows, "deep_scratch": sum(sum(1 for i in l["ins"] if i.startswith("scratch_")) for l in loops.values() if l["depth"] >= 2)})
    return out


if __name__ == "__main__":
    for k in walk_steps(open(sys.argv[1]).read(), sys.argv[2] if len(sys.argv) > 2 else ""):
        print(k["name"])
        for l in k["loops"]:
            print("   %-10s depth %d  instr %3d  VALU %3d  LDS %2d  SALU %2d  leaf-bit compares %d  scratch %d" % (
                l["header"], l["depth"], l["instr"], l["valu"], l["lds"], l["salu"], l["cmp_leaf"], l["scratch"]))
            r = l["rest"]
            print("   %-10s   back edge %s (%s)" % ("", " ".join(l["back_edge"]) or "none found", "scalar condition" if l["back_edge_scalar"] else "not a scalar condition"))
            if r: print("   %-10s   rest of the walk, %s depth %d:  instr %3d  VALU %3d  LDS %2d  SALU %2d" % ("", r["header"], r["depth"], r["instr"], r["valu"], r["lds"], r["salu"]))
            if "-v" in sys.argv:
                for i in l["ins"]: print("        " + i)
                for i in (r["ins"] if r else []): print("      rest: " + i)
