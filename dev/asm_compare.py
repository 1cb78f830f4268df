#!/usr/bin/env python3
"""Compare the device assembly of two trees kernel by kernel.

    make -C <tree>/deeplearningrecommendationsystem_amd/csrc build/gemm_dlds.s ...   (in both trees)
    dev/asm_compare.py <parent csrc/build> <head csrc/build> gemm_dlds gemm_dlds_dx ...

Per file: the kernel symbols of both sides, and for every kernel LDS bytes, scratch bytes, occupancy, SGPRs, VGPRs and
instruction count as the compiler's own trailer comments give them (a figure the trailer lacks prints as None).  A kernel's stream is everything from its label to
its .Lfunc_end with .file / .loc / .ident lines dropped; streams that differ in any way (register numbers included) are
listed with both sides' figures.  Exit status 1 when the symbol sets, or LDS / scratch / occupancy of any kernel, differ.
"""
import re
import sys

TRAILER = {"lds": r"; LDSByteSize: (\d+)", "scratch": r"; ScratchSize: (\d+)", "occ": r"; Occupancy: (\d+)",
           "sgpr": r"; TotalNumSgprs: (\d+)", "vgpr": r"; NumVgprs: (\d+)", "agpr": r"; NumAgprs: (\d+)"}


def kernels(path):
    out, name, body, kernel, open_ = {}, None, [], False, False
    lines = open(path).read().split("\n")
    for i, line in enumerate(lines):
        if re.match(r"\s*\.(file|loc|ident)\b", line):
            continue
        m = re.match(r"(\w+):\s*; @\1$", line)
        if m:
            name, body, kernel, open_ = m.group(1), [], False, True
        elif name and line.startswith(".Lfunc_end"):
            tail = "\n".join(lines[i:i + 40])
            info = {k: int(re.search(p, tail).group(1)) for k, p in TRAILER.items() if re.search(p, tail)}
            info["insts"] = sum(1 for b in body if re.match(r"\t[a-z]\w+", b))
            info["body"] = body
            if kernel:
                out[name] = info
            name = None
        elif name and (line.startswith("\t.section\t.rodata") or ".amdhsa_kernel " + name in line):
            kernel |= ".amdhsa_kernel " in line
            open_ = False     # the kernel descriptor follows: not part of the instruction stream
        elif name and open_:
            body.append(line)
    return out


def main():
    parent_dir, head_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = False
    for f in files:
        p, h = kernels(f"{parent_dir}/{f}.s"), kernels(f"{head_dir}/{f}.s")
        same_syms = sorted(p) == sorted(h)
        bad |= not same_syms
        changed = [k for k in sorted(p) if k in h and p[k]["body"] != h[k]["body"]]
        print(f"{f}: {len(p)} kernels, symbols {'identical' if same_syms else 'DIFFER'}, "
              f"instructions {sum(v['insts'] for v in p.values())} -> {sum(v['insts'] for v in h.values())}, "
              f"{len(changed)} streams differ")
        for k in sorted(set(p) ^ set(h)):
            print(f"  only in {'parent' if k in p else 'head'}: {k}")
        for k in sorted(set(p) & set(h)):
            res = [(x, p[k].get(x), h[k].get(x)) for x in ("lds", "scratch", "occ") if p[k].get(x) != h[k].get(x)]
            if res:
                bad = True
                print(f"  RESOURCES DIFFER {k}: " + ", ".join(f"{x} {a} -> {b}" for x, a, b in res))
        for k in changed:
            a, b = p[k], h[k]
            print(f"  {k}\n    insts {a['insts']} -> {b['insts']}  sgpr {a.get('sgpr')} -> {b.get('sgpr')}  "
                  f"vgpr {a.get('vgpr')} -> {b.get('vgpr')}  agpr {a.get('agpr')} -> {b.get('agpr')}  lds {a.get('lds')}  "
                  f"scratch {a.get('scratch')}  occupancy {a.get('occ')}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
