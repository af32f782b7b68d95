#!/usr/bin/env python3
"""tools/kernel_isa_diff.py [--show] old.s new.s [more_new.s ...] -- the compiler's assembly of two builds, compared kernel by kernel: prints
the kernels whose instruction streams differ or that have no counterpart; no GPU.  A kernel's stream is its lines without comments,
directives and metadata, with mangled symbols replaced by a placeholder and the .LBB label numbers counted from the kernel's first.
A kernel has a counterpart when a kernel of the other build has its name or, failing that, its stream (a kernel that was only renamed).
What is left over on both sides is paired by likeness, and the pairs are printed with the number of lines that differ (--show: the lines).
The .s files: the flags of tools/kernel_resources.sh with -S instead of -c, e.g.
    hipcc <flags> --offload-arch=gfx950 --cuda-device-only --no-gpu-bundle-output -S restir.hip -o new.s"""
import difflib, re, sys

def kernels(paths):
    out, name, labels = {}, None, {}
    for line in (l for p in paths for l in open(p)):
        line = line.split(";")[0].split("//")[0].rstrip()
        m = re.match(r"(\w+):$", line)
        if m: name, labels = m.group(1), {}; out[name] = []; continue
        if re.match(r"\s*\.(end_amdhsa_kernel|section)", line): name = None
        if name is None or not line.strip() or re.match(r"\s*\.(?!LBB)", line): continue
        line = re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), line)
        out[name].append(re.sub(r"_Z\w+", "SYM", " ".join(line.split())))
    return {k: tuple(v) for k, v in out.items() if v}

args = [a for a in sys.argv[1:] if a != "--show"]
old, new = kernels(args[:1]), kernels(args[1:])
same = [k for k in old if new.get(k) == old[k]]
streams = {v: k for k, v in new.items() if k not in old}
renamed = {k: streams[v] for k, v in old.items() if k not in same and v in streams}
left_old = [k for k in old if k not in same and k not in renamed]
left_new = [k for k in new if k not in same and k not in renamed.values() and not (k not in old and new[k] in old.values())]
for k in left_old:
    best = max(left_new, key=lambda n: difflib.SequenceMatcher(None, old[k], new[n], autojunk=False).quick_ratio(), default=None)
    if best is None: print("NO COUNTERPART (old)  %s" % k); continue
    d = [l for l in difflib.unified_diff(old[k], new[best], lineterm="", n=0) if l[0] in "+-" and l[:3] not in ("+++", "---")]
    print("DIFFERS  %d -> %d instructions, %d lines removed, %d added\n    old %s\n    new %s" % (len(old[k]), len(new[best]), sum(l[0] == "-" for l in d), sum(l[0] == "+" for l in d), k, best))
    if "--show" in sys.argv: print("\n".join("        " + l for l in d))
    left_new.remove(best)
for k in left_new: print("NO COUNTERPART (new)  %s" % k)
print("%d kernels identical under their name, %d identical under another name, of %d old and %d new" % (len(same), len(renamed), len(old), len(new)))
