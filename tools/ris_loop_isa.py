#!/usr/bin/env python3
"""tools/ris_loop_isa.py [file.s ...] -- the instructions a wave executes per pass of every innermost loop of one kernel, counted in the
compiler's assembly (no GPU needed): all of them, without s_nop / s_waitcnt, the vector ones, and the 64-bit multiply-adds.

Default kernel: k_ris_lds<false, 0> (minstd, the light history off), whose three loops are, in the order printed, the candidate loop of a wave with metallic lanes, the
candidate loop of a wave of Lambertian pixels alone, and the draws-only loop of an empty light table (EXPERIMENTS.md, "One range guard per
RIS candidate" and "The generator on its state minus one": 331 / 202 / 34 before the latter, 321 / 191 / 28 after it).  A loop's body is
the lines from its header label to its last back-branch: the path on which no branch but the loop's own is taken, i.e. every guard
answers "in range" and every exec-masked region runs -- the re-evaluation of a candidate sits behind the back-branch and is not counted.

The assembly of a source, with the library's flags (restir_amd/csrc/Makefile):
    hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize \\
          --offload-arch=gfx950 --cuda-device-only -S restir_amd/csrc/restir.hip -o restir.s
    tools/ris_loop_isa.py restir.s            (--kernel MANGLED_NAME for another kernel)"""
import re
import sys

DEFAULT = "_ZN12_GLOBAL__N_19k_ris_ldsILb0ELi0EEEvN2rs8DevSceneENS1_10SurfPlanesEiiiiNS1_10RisWinnersIXT0_EEE"     # k_ris_lds<false, 0>


def kernel(path, name):
    lines = open(path).read().split("\n")
    s = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    e = next(i for i in range(s, len(lines)) if lines[i].startswith("\t.size\t" + name))
    return lines[s:e]


def is_instruction(l):
    return l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;") and l.strip() != ""


def loops(body):
    out = []
    for i, l in enumerate(body):
        m = re.match(r"(\.LBB\d+_\d+):.*Inner Loop Header", l)
        if not m:
            continue
        h = m.group(1)
        j = next((k for k in range(len(body) - 1, i, -1) if re.search(r"s_c?branch\w* " + re.escape(h) + r"$", body[k].rstrip())), None)
        if j is None:
            continue
        ins = [x for x in body[i:j + 1] if is_instruction(x)]
        out.append((h, len(ins), sum(not re.match(r"\ts_(nop|waitcnt)", x) for x in ins), sum(x.startswith("\tv_") for x in ins),
                    sum("v_mad_u64_u32" in x for x in ins)))
    return out


def main(argv):
    name = DEFAULT
    if "--kernel" in argv:
        i = argv.index("--kernel")
        name = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    for path in argv:
        print(path)
        for r in loops(kernel(path, name)):
            print("   loop %s: instructions %d, without s_nop / s_waitcnt %d, vector %d, v_mad_u64_u32 %d" % r)


if __name__ == "__main__":
    main(sys.argv[1:])
