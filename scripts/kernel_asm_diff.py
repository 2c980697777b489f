#!/usr/bin/env python3
"""Two directories of device-only assembly listings (hipcc --cuda-device-only -S, one <file>.<build>.s per translation unit and build)
compared KERNEL BY KERNEL: for every listing the sha256 of both sides, the number of kernels, and for each kernel whose text differs the
changed line count (unified diff, +/- lines) with SGPRs / VGPRs / spills / scratch of both sides (profiles/region_box.md).
A kernel whose argument list changed has another symbol: such kernels are paired by their name and template arguments (SAME NAME, NEW
ARGUMENTS) and their figures compared; what is left on one side only is listed as DISAPPEARED / APPEARED — an appeared kernel with
its figures, of which a spill or scratch counts as worse (profiles/cg_kernels.md).
Exit code 0 when no kernel's register, spill or scratch figures got worse and no listing is missing.
usage: kernel_asm_diff.py DIR_PARENT DIR_CHANGE"""
import difflib, hashlib, os, re, subprocess, sys


def kernels(path):
    txt = open(path).read()
    body = {}
    # a kernel's text: from its label to its .Lfunc_end; its figures: the .amdhsa_ block and the metadata entry
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        body[m.group(1)] = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))   # (block labels carry the kernel's ordinal in the file: a kernel added above renumbers them)
    meta = {}
    for b in txt.split("  - .agpr_count:")[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, b) or [None, "-"])[1]
        meta[g("name")] = tuple(g(k) for k in ("sgpr_count", "vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size"))
    return {k: (v, meta[k]) for k, v in body.items() if k in meta}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"\(anonymous namespace\)::", "", n).replace("void ", "") for n in out]


def main(a, b):
    worse = 0
    for f in sorted(set(os.listdir(a)) | set(os.listdir(b))):
        if not f.endswith(".s"):
            continue
        pa, pb = os.path.join(a, f), os.path.join(b, f)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print("MISSING", f); worse += 1
            continue
        ha, hb = (hashlib.sha256(open(p, "rb").read()).hexdigest()[:16] for p in (pa, pb))
        ka, kb = kernels(pa), kernels(pb)
        diff = [k for k in sorted(set(ka) | set(kb)) if k not in ka or k not in kb or ka[k] != kb[k]]
        print("%-28s %s %s kernels %3d / %3d  %s" % (f, ha, hb, len(ka), len(kb),
              "byte-identical" if ha == hb else "%d kernels differ" % len(diff) if diff else "no kernel differs (text outside the kernels)"))
        names = dict(zip(diff, demangle(diff)))
        stem = lambda k: names[k].split("(")[0]
        one = {side: {} for side in "ab"}
        for k in diff:
            if k not in ka or k not in kb:
                one["a" if k in ka else "b"].setdefault(stem(k), []).append(k)
        pairs = [(k, k) for k in diff if k in ka and k in kb]
        for s in sorted(set(one["a"]) | set(one["b"])):
            a1, b1 = one["a"].get(s, []), one["b"].get(s, [])
            if len(a1) == len(b1) == 1:
                pairs.append((a1[0], b1[0]))
                continue
            for k in a1:
                print("    DISAPPEARED", names[k])
            for k in b1:   # a new kernel has no parent to compare with: its figures are printed, and a spill or scratch counts as worse
                m = kb[k][1]
                print("    APPEARED   ", names[k], "| sgpr vgpr sgpr-spill vgpr-spill scratch:", " ".join(m))
                worse += any(y != "-" and int(y) > 0 for y in m[2:])
        for k, k2 in pairs:
            d = [l for l in difflib.unified_diff(ka[k][0].split("\n"), kb[k2][0].split("\n"), lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            print("    %-90s lines %5d | %d changed | sgpr vgpr sgpr-spill vgpr-spill scratch: %s -> %s%s" % (
                names[k][:90], ka[k][0].count("\n"), len(d), " ".join(ka[k][1]), " ".join(kb[k2][1]), "" if k == k2 else "   SAME NAME, NEW ARGUMENTS"))
            worse += any(y != "-" and int(y) > int(x) for x, y in zip(ka[k][1], kb[k2][1]))
    print("RESULT", "no figure worse" if not worse else "%d kernels WORSE or listings missing" % worse)
    return 1 if worse else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
