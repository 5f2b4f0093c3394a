#!/usr/bin/env python3
"""Are two builds' kernels the same machine code?  For changes that are meant to touch host code only.

    tools/device_asm_diff.py OLD.s NEW.s [--allow KERNEL_SUBSTRING ...]

OLD.s / NEW.s: device assembly of csrc/mlp_hip.hip as tools/isa_mix.py makes it
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only [-DDVDA_BOUNDS=1]).  Each file is cut at its kernel
symbols; a kernel's text is everything from its label to its `-- End function` line, comments dropped: the code, the
`.amdhsa_*` resource block and the `.set` resource values.  Labels the compiler numbers by the function's position in
the file (.LBB12_3, .Ltmp45, .Lfunc_end12) are rewritten without that number: moving code between headers changes
nothing else.  Exit status 1 if the sets of kernel names differ or any kernel's text does, except kernels named by
--allow, whose diff is printed."""
import difflib
import re
import sys

KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
NUMBERED = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"),
            (re.compile(r"\.L(tmp|JTI|CPI|_?\$local)\d*(_\d+)?"), r".L\1")]


def kernels(path):
    """name -> normalised text of the kernel"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in map(KERNEL.match, lines) if m]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if "-- End function" in lines[i])
        text = []
        for ln in lines[start:end + 1]:
            ln = ln.split(";")[0].rstrip() if not ln.lstrip().startswith(".amdhsa") else ln.rstrip()
            for pat, rep in NUMBERED:
                ln = pat.sub(rep, ln)
            if ln.strip():
                text.append(ln)
        out[name] = text
    return out


def main(argv):
    allow = []
    if "--allow" in argv:
        i = argv.index("--allow")
        allow, argv = argv[i + 1:], argv[:i]
    old, new = kernels(argv[1]), kernels(argv[2])
    bad = 0
    for name in sorted(set(old) ^ set(new)):
        print("only in %s: %s" % ("OLD" if name in old else "NEW", name))
        bad += 1
    same = 0
    for name in sorted(set(old) & set(new)):
        if old[name] == new[name]:
            same += 1
            continue
        allowed = any(a in name for a in allow)
        print("%s: %s" % ("differs (allowed)" if allowed else "DIFFERS", name))
        sys.stdout.write("\n".join(list(difflib.unified_diff(old[name], new[name], "OLD", "NEW", lineterm="", n=2))[:200]) + "\n")
        bad += 0 if allowed else 1
    print("%d kernels in OLD, %d in NEW, %d identical" % (len(old), len(new), same))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
