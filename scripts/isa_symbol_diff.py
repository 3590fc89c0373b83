"""Which kernel symbols did a change touch?  Two modes:

    python scripts/isa_symbol_diff.py list OUTDIR          # hipcc --cuda-device-only -S of every kernel unit of THIS tree (build.py's flags) into OUTDIR
    python scripts/isa_symbol_diff.py compare DIR_A DIR_B  # symbol by symbol: instruction stream, kernel descriptor, metadata entry

Run `list` in a checkout of the parent commit and in the working tree, then `compare` the two directories.  Symbols are matched by mangled name;
the numbers the listing gives functions in order of emission (.LBB<fn>_<block>, "Header=BB<fn>_<n>" in comments) are dropped, so that adding a
kernel to a unit does not rename its neighbours' labels.  Prints the symbols of A that changed or vanished and the symbols new in B (demangled
where c++filt exists).  DESIGN.md section 10 quotes its result for the list-driven frame-group kernels."""
import concurrent.futures as cf
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def listings(out):
    sys.path.insert(0, ROOT)
    from tracerboy_amd import build as b
    os.makedirs(out, exist_ok=True)

    def one(src):
        cmd = [b.HIPCC] + b.COMMON + list(b.device_flags(src)) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o",
                                                                  os.path.join(out, os.path.basename(src) + ".s")]
        return src, subprocess.run(cmd, capture_output=True, text=True).returncode
    with cf.ThreadPoolExecutor(4) as ex:
        for src, rc in ex.map(one, b.KERNEL_SRCS):
            print(src, "ok" if rc == 0 else "FAILED (%d)" % rc, flush=True)


def split(path):
    """symbol -> text of its function body (from its label to .Lfunc_end), and the metadata entries keyed by .name"""
    txt = open(path).read()
    funcs = {}
    for m in re.finditer(r'^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:', txt, re.S | re.M):
        funcs[m.group(1)] = m.group(2)
    meta = {}
    md = txt[txt.find('amdhsa.kernels:'):] if 'amdhsa.kernels:' in txt else ''
    md = re.split(r'\n(?=amdhsa\.\w+:)', md)[0]   # the block ends at the next top-level key: whichever entry comes last would otherwise carry the file's trailer
    for blk in re.split(r'\n  - ', md)[1:]:
        n = re.search(r'\.name:\s+(\S+)', blk)
        if n: meta[n.group(1)] = blk
    kd = {m.group(1): m.group(2) for m in re.finditer(r'\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel', txt, re.S)}
    return funcs, meta, kd
def norm(body):
    # the listing numbers functions in order of emission (.LBB<fn>_<block>, .LJTI<fn>_<n>, "Header=BB<fn>_<n>" in comments): drop the function number
    body = re.sub(r'(\.L)?(BB|JTI)\d+_(\d+)', r'\1\2_\3', body)
    body = re.sub(r'\.L(func_begin|func_end|tmp)\d+', r'.L\1', body)
    return re.sub(r'[ \t]+', ' ', body)


def compare(a, b):
    tot = same = 0; new = []; changed = []
    for f in sorted(os.listdir(a)):
        fa, ma, ka = split(os.path.join(a, f)); fb, mb, kb = split(os.path.join(b, f))
        for sym in fa:
            tot += 1
            if sym not in fb: changed.append((f, sym, 'missing')); continue
            if norm(fa[sym]) != norm(fb[sym]): changed.append((f, sym, 'text')); continue
            if sym in ma and ma[sym] != mb.get(sym): changed.append((f, sym, 'metadata')); continue
            if sym in ka and ka[sym] != kb.get(sym): changed.append((f, sym, 'descriptor')); continue
            same += 1
        new += [(f, s) for s in fb if s not in fa]
    print('parent symbols', tot, 'unchanged', same, 'changed', len(changed), 'new', len(new))
    for c in changed[:40]: print('CHANGED', c)
    dem = [s for _, s in new] if not shutil.which('c++filt') else subprocess.run(['c++filt'], input='\n'.join(s for _, s in new), capture_output=True, text=True).stdout.split('\n')
    for (f, s), d in zip(new, dem): print('NEW', f, d[:220])
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "list":
        listings(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
