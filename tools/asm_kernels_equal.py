#!/usr/bin/env python3
"""Are two device assemblies (hipcc --cuda-device-only -S) the same code, function by function?

    tools/asm_kernels_equal.py parent.s branch.s

A plain `diff` of two such files is empty only if the functions are also EMITTED in the same order, and hipcc emits template
kernels in the order in which host code first names them: moving a launch from one host function to another reorders the file
and renumbers every local label (.LBB<function index>_<block>) without touching an instruction.  This compares what the order
cannot change: for every function its text (instructions, operands, directives, the .amdhsa_kernel descriptor and the resource
comments behind it) with the function index taken out of the local labels, and its entry in the code-object metadata.  Lines
naming the per-file __hip_cuid_ symbol are ignored.  Exit status 0: the same set of functions, each with identical text.
"""
import re
import sys

BEGIN = re.compile(r"^\t\.section\t\.text\.([A-Za-z0-9_$.]+),")
LABEL = re.compile(r"\.L(BB|JTI|CPI|tmp)\d+_|\.Lfunc_(begin|end)\d+")
LOOP = re.compile(r"(Header=|Child Loop |Parent Loop )BB\d+_")      # the same index in the loop comments


def unnumber(line):      # ... and the padding in front of a comment, which follows the label's width
    line = LABEL.sub(lambda m: ".L%s_" % m.group(1) if m.group(1) else ".Lfunc_%s" % m.group(2), line)
    return re.sub(r"[ \t]+;", " ;", LOOP.sub(r"\1BB_", line))


def split(path):
    """-> (text before the first function, {function: lines}, {kernel: metadata lines}, the rest, emission order)"""
    head, funcs, meta, rest, order = [], {}, {}, [], []
    cur, where = head, "text"
    with open(path) as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            if where == "text":
                m = BEGIN.match(line)
                if m and m.group(1) in funcs:        # back from the kernel descriptor's .rodata
                    cur = funcs[m.group(1)]
                elif m:
                    cur = funcs[m.group(1)] = []
                    order.append(m.group(1))
                elif line.startswith("\t.section\t.AMDGPU.gpr_maximums"):      # behind the last function
                    cur = rest
                elif line.startswith("\t.amdgpu_metadata"):
                    where, cur = "meta", rest
                cur.append(unnumber(line))
            elif where == "meta":
                if line.startswith("  - "):          # one entry of amdhsa.kernels; keyed by its .name below
                    cur = []
                    meta[len(meta)] = cur
                elif not line.startswith(" ") and meta:      # amdhsa.target, amdhsa.version, .end_amdgpu_metadata
                    where, cur = "tail", rest
                cur.append(line)
            else:
                rest.append(line)
    named = {}
    for entry in meta.values():
        name = [l.split()[1] for l in entry if l.strip().startswith(".name:")]
        named[name[0]] = entry
    return head, funcs, named, rest, order


def main(a, b):
    A, B = split(a), split(b)
    bad = 0
    for what, x, y in (("function", A[1], B[1]), ("metadata entry", A[2], B[2])):
        for name in sorted(set(x) | set(y)):
            if name not in x or name not in y:
                print("%s only in %s: %s" % (what, b if name in y else a, name))
                bad += 1
            elif x[name] != y[name]:
                print("%s differs: %s" % (what, name))
                bad += 1
    if A[0] != B[0] or A[3] != B[3]:
        print("the text outside the functions differs")
        bad += 1
    kernels = sum(1 for lines in A[1].values() if any(l.startswith("\t.amdhsa_kernel ") for l in lines))
    print("%d functions (%d kernels) in %s, %d in %s; emitted in %s order; %s" % (
        len(A[1]), kernels, a, len(B[1]), b, "the same" if A[4] == B[4] else "ANOTHER",
        "every function and metadata entry identical" if not bad else "%d differences" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
