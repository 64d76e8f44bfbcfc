#!/usr/bin/env python3
"""Device-code comparison of two builds of csrc/*.hip, kernel by kernel.

    isa_diff.py emit <repo root> <out dir>     one .s per csrc/*.hip: build.py's FLAGS (+ EXTRA_FLAGS) -S --cuda-device-only
    isa_diff.py compare <dir A> <dir B>        compare two such directories

compare looks at the whole library, not at files: a kernel may move between translation units.  For every
`.amdhsa_kernel` symbol it takes the instruction stream (from the symbol's label to its descriptor) and the
`.amdhsa_*` descriptor block (register counts, LDS and scratch size), and normalises the compiler-numbered local labels
(`.LBB<n>_<m>`, `.Lfunc_end<n>`), whose <n> is the function's position in its translation unit.  Exit status 0 when the
symbol sets are equal and every kernel is identical.
"""
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor


def emit(root, out):
    spec = importlib.util.spec_from_file_location("vitseg_build", os.path.join(root, "visiontransformer_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    os.makedirs(out, exist_ok=True)

    def one(src):
        name = os.path.basename(src)
        cmd = [b.HIPCC] + b.FLAGS + b.EXTRA_FLAGS.get(name, []) + ["-S", "--cuda-device-only", src, "-o",
                                                                    os.path.join(out, name[:-4] + ".s")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")

    with ThreadPoolExecutor(max_workers=int(os.environ.get("MAX_JOBS", "8"))) as ex:
        list(ex.map(one, b.sources()))


LOCAL = re.compile(r"\.L(BB|func_end)(\d+)")


def kernels(d):
    """symbol -> (file, normalised text: body lines + descriptor lines)"""
    out = {}
    for f in sorted(os.listdir(d)):
        if not f.endswith(".s"):
            continue
        lines = open(os.path.join(d, f)).read().split("\n")
        label = {}
        for i, l in enumerate(lines):
            m = re.match(r"([A-Za-z_$][\w$.]*):", l)
            if m:
                label[m.group(1)] = i
        i = 0
        while i < len(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
            if not m:
                i += 1
                continue
            sym = m.group(1)
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            desc = [l.strip() for l in lines[i + 1:j]]
            e = j   # the descriptor sits between the code and the function's end label
            while not lines[e].startswith(".Lfunc_end"):
                e += 1
            fn = LOCAL.search(lines[e]).group(2)
            body = []
            for l in lines[label[sym] + 1:i]:
                l = l.split(";")[0].rstrip()   # comments carry no code
                if l:
                    body.append(LOCAL.sub(lambda x: f".L{x.group(1)}#" if x.group(2) == fn else x.group(0), l))
            if sym in out:
                raise RuntimeError(f"{sym} emitted twice ({out[sym][0]}, {f})")
            out[sym] = (f, body + desc)
            i = j
    return out


def compare(da, db):
    a, b = kernels(da), kernels(db)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    common = sorted(set(a) & set(b))
    differ = [s for s in common if a[s][1] != b[s][1]]
    moved = sum(1 for s in common if a[s][0] != b[s][0])
    print(f"kernels in A: {len(a)}   kernels in B: {len(b)}   in both: {len(common)}")
    print(f"identical (instruction stream + .amdhsa descriptor): {len(common) - len(differ)}")
    print(f"emitted by a different file in B: {moved}")
    for f in sorted({v[0] for v in a.values()} | {v[0] for v in b.values()}):
        na, nb = sum(1 for v in a.values() if v[0] == f), sum(1 for v in b.values() if v[0] == f)
        if na != nb:
            print(f"  {f}: {na} -> {nb}")
    print(f"only in A: {len(only_a)}")
    for s in only_a:
        print("  " + s)
    print(f"only in B: {len(only_b)}")
    for s in only_b:
        print("  " + s)
    print(f"differing: {len(differ)}")
    for s in differ:
        la, lb = a[s][1], b[s][1]
        n = sum(1 for x, y in zip(la, lb) if x != y) + abs(len(la) - len(lb))
        print(f"  {s}: {len(la)} -> {len(lb)} lines, {n} differ")
    return 0 if not (only_a or only_b or differ) else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
