#!/usr/bin/env python3
"""Wait states between an MFMA and the inline-asm VALU instructions that follow it, counted in hipcc's device assembly.

hipcc's hazard recogniser inserts the wait states an MFMA needs before a dependent instruction only for instructions it knows; an
instruction written as inline asm gets none.  f16x3.hip writes two v_mul_f32 and one v_sub_f32 that way.  For
every asm instruction this prints the smallest distance, in wait states (one per instruction in between, N + 1 for s_nop N), to an
earlier MFMA of the same straight-line stretch
  * whose C operand the asm instruction writes  (write after read;  a 4-pass MFMA needs 3),
  * whose result register it writes             (write after write; a 4-pass MFMA needs 7),
  * whose result register it reads, with no VALU rewrite in between (read after write: f16x3.hip must have none at all).
Back edges of loops are not followed: a stretch ends at a function label.  Exit status 1 if a distance is below its requirement.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S baler_amd/csrc/f16x3.hip -o f16x3.s
    python tools/asm_mfma_gaps.py f16x3.s
"""
import re
import sys

NEED = {"war": 3, "waw": 7}      # v_mfma_f32_16x16x32_f16: 4 passes
WINDOW = 40                      # wait states looked back: far beyond any requirement


def regs(op):
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", op)
    return {int(m.group(1))} if m else set()


def instructions(path):
    """(mnemonic, operands, inside inline asm) per instruction; ("LABEL", [name], False) at every function label."""
    out, in_asm = [], False
    for line in open(path):
        t = line.strip()
        if t.startswith(";;#ASMSTART"):
            in_asm = True
        elif t.startswith(";;#ASMEND"):
            in_asm = False
        elif re.match(r"^_Z\w+:", line):
            out.append(("LABEL", [line.split(":")[0]], False))
        elif line.startswith("\t") and t and t[0] not in ".;":
            parts = t.split(";")[0].strip().split(None, 1)
            out.append((parts[0], [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else [], in_asm))
    return out


def main(path):
    ins = instructions(path)
    best = {"war": None, "waw": None, "raw": None}
    n_asm = 0
    for j, (mn, ops, in_asm) in enumerate(ins):
        if not in_asm or not ops:
            continue
        n_asm += 1
        dst = regs(ops[0])
        live = set().union(*[regs(o) for o in ops[1:]]) if len(ops) > 1 else set()
        ws = 0
        for i in range(j - 1, -1, -1):
            pm, po, _ = ins[i]
            if pm == "LABEL" or ws > WINDOW:
                break
            if pm.startswith("v_mfma"):
                for kind, hit in (("war", regs(po[3]) & dst), ("waw", regs(po[0]) & dst), ("raw", regs(po[0]) & live)):
                    if hit and (best[kind] is None or ws < best[kind]):
                        best[kind] = ws
            elif pm.startswith("v_") and po:
                live -= regs(po[0])
            ws += int(po[0], 0) + 1 if pm == "s_nop" else 1
    print(f"{n_asm} inline-asm instructions, {sum(1 for i in ins if i[0].startswith('v_mfma'))} MFMAs")
    ok = True
    for kind, text in (("war", "write after read "), ("waw", "write after write"), ("raw", "read after write ")):
        b = best[kind]
        need = NEED.get(kind)
        good = b is None or (need is not None and b >= need)
        ok &= good
        print(f"{text}: smallest distance {'none within ' + str(WINDOW) if b is None else b} wait states"
              f" ({'needs ' + str(need) if need is not None else 'must not occur'}){'' if good else '   <-- HAZARD'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
