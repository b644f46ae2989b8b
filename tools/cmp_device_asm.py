"""Compare the device code of two builds of one .hip file, whatever the order the kernels come in.

    hipcc <the Makefile's flags> --cuda-device-only -S rp_ring.hip -o a.s    (on each tree)
    python tools/cmp_device_asm.py a.s b.s

A refactor of host code must leave the device assembly alone, but the compiler emits kernels in the
order host code first names them, so two such files can differ as a whole. This compares them
piece by piece. A piece is one function, from its .section / .globl lines to the line before the
next function's, with the function's emission ordinal taken out of its local labels
(.LBB<ordinal>_<n>, .Lfunc_end<ordinal>), the assembler comments (which cite those labels) dropped
and the name of __hip_cuid_<hash of the source file> made equal. The metadata at the end is
compared as the sorted list of its per-kernel entries. Exit status 0: the same functions, every
piece identical.
"""
import re
import sys


def pieces(path):
    txt = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read())
    lines = txt.split("\n")
    begins = [i for i, l in enumerate(lines) if "; -- Begin function " in l]
    starts = []
    for i in begins:
        s = i
        while s > 0 and re.match(r"\s*\.(section|protected|weak|hidden|text)\b", lines[s - 1]):
            s -= 1
        starts.append(s)
    md = next(i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata")
    out = {"<head>": "\n".join(lines[: starts[0]])}
    for n, (s, b) in enumerate(zip(starts, begins)):
        e = starts[n + 1] if n + 1 < len(starts) else md
        name = lines[b].split("; -- Begin function ")[1].strip()
        body = "\n".join(lines[s:e])
        body = re.sub(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b", lambda m: ".L" + m.group(1) + (m.group(2) or ""), body)
        body = re.sub(r"[ \t]*;.*", "", body)
        assert name not in out, name
        out[name] = body
    out["<metadata>"] = "\n".join(sorted(re.split(r"\n(?=  - \.)", "\n".join(lines[md:]))))
    return out


if __name__ == "__main__":
    a, b = pieces(sys.argv[1]), pieces(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    diff = [k for k in a if k in b and a[k] != b[k]]
    print("functions: %d and %d; only in the first: %s; only in the second: %s; differing: %s"
          % (len(a) - 2, len(b) - 2, only_a, only_b, diff))
    print("emission order %s" % ("equal" if list(a) == list(b) else "differs"))
    sys.exit(1 if (only_a or only_b or diff) else 0)
