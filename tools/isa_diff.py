#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (CPU only).

usage: tools/isa_diff.py a.s b.s [--show NAME]

a.s / b.s: gfx950 assembly of kapre_amd/csrc/kapre_hip.hip, i.e. the flags of kapre_amd/build.py with
`--cuda-device-only -S` instead of `-fPIC -shared`.  Per kernel symbol three texts are compared: the body, the kernel
descriptor (.amdhsa_kernel block) and the metadata entry (VGPR / SGPR / LDS / scratch sizes, arguments).  Local labels
(.LBB*, .Ltmp*, .Lfunc_end*) are renamed by order of appearance and comments are dropped, so the textual order of the
kernels and the numbering of their labels do not matter.  Prints the kernel counts, the symbols present on one side
only and the names of the differing kernels; --show NAME adds a unified diff of one kernel.  Exit status 1 on any
difference.
"""
import difflib
import re
import sys

_LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def _normalise(lines):
    """Drop comments and blank lines, rename local labels by order of appearance."""
    names, out = {}, []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if ln.strip():
            out.append(_LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln))
    return out


def kernels(text):
    """{symbol: normalised lines of body + descriptor + metadata entry, each part under a heading}"""
    lines = text.splitlines()
    parts, start = {}, {}
    for i, ln in enumerate(lines):
        m = re.match(r"([A-Za-z_][\w$.]*):", ln)
        if m:
            start[m.group(1)] = i
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m and m.group(1) in start:
            name = m.group(1)
            end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
            parts[name] = ["== body"] + _normalise(lines[start[name] + 1:i]) + \
                          ["== descriptor"] + _normalise(lines[i + 1:end])
    # metadata: one YAML list entry per kernel under amdhsa.kernels
    entries = []
    for ln in lines[next((i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")), len(lines)) + 1:]:
        if ln.startswith("  - "):
            entries.append([])
        elif not ln.startswith("   "):
            break
        entries[-1].append(ln.rstrip())
    for e in entries:
        name = next((m.group(1) for m in (re.match(r"\s+\.name:\s+(\S+)", ln) for ln in e) if m), None)
        if name in parts:
            parts[name] += ["== metadata"] + e
    return parts


def compare(text_a, text_b):
    """-> (kernels of a, kernels of b, symbols only in a, symbols only in b, names of differing kernels)"""
    a, b = kernels(text_a), kernels(text_b)
    return a, b, sorted(set(a) - set(b)), sorted(set(b) - set(a)), sorted(k for k in a if k in b and a[k] != b[k])


def main(argv):
    show = None
    if "--show" in argv:
        i = argv.index("--show")
        show = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    if len(argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    a, b, only_a, only_b, differ = compare(open(argv[0]).read(), open(argv[1]).read())
    print("kernels: %d in %s, %d in %s" % (len(a), argv[0], len(b), argv[1]))
    print("only in %s: %d" % (argv[0], len(only_a)))
    for k in only_a:
        print("  " + k)
    print("only in %s: %d" % (argv[1], len(only_b)))
    for k in only_b:
        print("  " + k)
    print("differing: %d" % len(differ))
    for k in differ:
        print("  " + k)
    if show:
        if show not in a or show not in b:
            print("--show: %s is not in both files" % show, file=sys.stderr)
            return 2
        sys.stdout.writelines(difflib.unified_diff([x + "\n" for x in a[show]], [x + "\n" for x in b[show]],
                                                   argv[0], argv[1]))
    return 1 if (only_a or only_b or differ) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
