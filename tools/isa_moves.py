"""tools/isa_moves.py KERNEL.s MAM_SM_HPP [SYMBOL ...] -- the static table of
what k_mam_sm's instruction stream spends on handing values between blocks:
moves by kind, selects, scalar exec-mask work, branches, the structurizer's
Flow blocks, blocks that hold nothing but moves and lane-mask bookkeeping, and the
"implicit-def" annotations (a value undefined on one path into a merge), then
registers / scratch / occupancy, and moves and VALU per source region
(isa_regions.py's attribution: the outermost mam_sm.hpp line of the loop body).

SYMBOL is a substring of a kernel's mangled name, as for isa_waits.py; with
none given, the three production instantiations: GEO 150, GEO 100 and the
generic packed kernel.  The .s comes from

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude --cuda-device-only \\
          -S -gline-tables-only -fno-discard-value-names smash-paper_amd/csrc/mam.hip

(-fno-discard-value-names keeps the block names, so the Flow blocks show)

It classifies moves, selects, branches and exec-mask operations only; every
other instruction counts as plain VALU / SALU.  Diagnostic tooling."""
import re
import sys
from collections import Counter

from isa_waits import function_lines

DEFAULTS = [("geo150", "ImLi64ELb1ELb0ELb1ELi150E"), ("geo100", "ImLi64ELb1ELb0ELb1ELi100E"),
            ("packed", "ImLi64ELb1ELb0ELb1ELi0E")]
MOVE = re.compile(r"^v_mov_b(32|64)")
VREG = re.compile(r"^v(\d+|\[\d+:\d+\])$")
EXEC_RESTORE = re.compile(r"^s_(or|mov|xor|andn2|and)_b64\s+exec\b")
MASK_OP = re.compile(r"^s_(or|mov|xor|andn2|and|orn2)_b64\b|^s_\w+_saveexec_b64\b")


def regions(src_path):
    """isa_regions.py's marks: (first line, name) of each consume case and decide block"""
    marks = []
    for i, l in enumerate(open(src_path).read().split("\n"), 1):
        m = re.search(r"case (S_[A-Z]+)|if \(st0 [=>]= (S_[A-Z]+)\)|if \(a == (A_[A-Z_]+)[ )]|(// ---------------- decide)|(for \(;;\) \{)", l)
        if m:
            marks.append((i, next(g for g in m.groups() if g)))
    body0 = next(i for i, n in marks if n.startswith("for"))

    def region(line):
        r = "loop-top"
        for i, n in marks:
            if i <= line:
                r = n
        return r
    return body0, region


def table(lines, sym, body0, region):
    a, b = function_lines(lines, sym)
    n = Counter()
    mv_region, valu_region = Counter(), Counter()
    cur = None          # source line the instruction is attributed to (None: no line in the loop body)
    blocks = []         # per basic block: list of instruction texts
    blk = []
    for l in lines[a:b]:
        if "\t.loc\t" in l:
            chain = [int(x) for x in re.findall(r"mam_sm\.hpp:(\d+):\d+", l)]
            outer = [x for x in chain if x >= body0]
            cur = outer[-1] if outer else None
            continue
        if re.match(r"^\.LBB\d+_\d+:", l) or l.startswith("; %bb."):
            blocks.append(blk)
            blk = []
            n["flow"] += "%Flow" in l
            continue
        if "; implicit-def: $vgpr" in l and "SGPR spill" not in l:
            n["implicit_def"] += 1
            continue
        if not re.match(r"^\t[a-z]", l):
            continue
        ins = l.split(";")[0].strip()
        op = ins.split()[0]
        blk.append(ins)
        where = region(cur) if cur is not None else "(no line in the loop body)"
        if op.startswith("v_"):
            n["valu"] += 1
            valu_region[where] += 1
            m = MOVE.match(op)
            if m:
                n["mov_b" + m.group(1)] += 1
                mv_region[where] += 1
                srcop = ins.split(",")[-1].strip()
                if VREG.match(srcop):
                    n["mov_reg"] += 1
                    n["mov_reg_b64"] += m.group(1) == "64"
                else:
                    n["mov_const"] += 1
            elif op.startswith("v_cndmask"):
                n["cndmask"] += 1
        elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop")):
            if op.startswith(("s_cbranch", "s_branch")):
                n["branch"] += 1
                continue
            n["salu"] += 1
            if "saveexec" in op:
                n["saveexec"] += 1
            elif EXEC_RESTORE.match(ins):
                n["exec_restore"] += 1
            if op == "s_or_b64":
                n["s_or_b64"] += 1
    blocks.append(blk)
    for bl in blocks:
        body = [i for i in bl if not i.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop"))]
        mv = [i for i in body if MOVE.match(i)]
        if mv and all(MOVE.match(i) or MASK_OP.match(i) for i in body):
            n["move_only_blocks"] += 1
            n["move_only_moves"] += len(mv)
    info = next((i for i in range(b, len(lines)) if lines[i].startswith("; Kernel info:")), None)
    regs = {}
    for l in (lines[info:info + 20] if info is not None else []):
        m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)", l)
        if m:
            regs[m.group(1)] = int(m.group(2))
    return lines[a].split(":")[0], n, regs, mv_region, valu_region


def show(name, n, regs, mv_region, valu_region):
    moves = n["mov_b32"] + n["mov_b64"]
    print(name)
    print("VALU                          %5d" % n["valu"])
    print("  v_mov_b32 / v_mov_b64       %5d / %d, together %d = %.0f %% of VALU"
          % (n["mov_b32"], n["mov_b64"], moves, 100.0 * moves / max(1, n["valu"])))
    print("  moves of a constant         %5d   (immediate or SGPR source)" % n["mov_const"])
    print("  register-to-register moves  %5d   of them %d 64-bit" % (n["mov_reg"], n["mov_reg_b64"]))
    print("  v_cndmask                   %5d" % n["cndmask"])
    print("SALU                          %5d" % n["salu"])
    print("  branches                    %5d   (counted apart from SALU)" % n["branch"])
    print("  s_*_saveexec                %5d" % n["saveexec"])
    print("  exec restores               %5d" % n["exec_restore"])
    print("  s_or_b64                    %5d" % n["s_or_b64"])
    print("Flow blocks                   %5d" % n["flow"])
    print("implicit-def $vgpr            %5d" % n["implicit_def"])
    print("move-only blocks              %5d   holding %d moves" % (n["move_only_blocks"], n["move_only_moves"]))
    print("VGPRs %d, AGPRs %d, SGPRs %d, scratch %d, occupancy %d" % (
        regs.get("NumVgprs", -1), regs.get("NumAgprs", -1), regs.get("TotalNumSgprs", -1),
        regs.get("ScratchSize", -1), regs.get("Occupancy", -1)))
    print("%-32s %6s %6s" % ("region", "moves", "VALU"))
    for r, c in sorted(valu_region.items(), key=lambda x: (-mv_region[x[0]], -x[1])):
        print("%-32s %6d %6d" % (r, mv_region[r], c))


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    lines = open(sys.argv[1]).read().split("\n")
    body0, region = regions(sys.argv[2])
    syms = [(s, s) for s in sys.argv[3:]] or DEFAULTS
    for k, (tag, sym) in enumerate(syms):
        if k:
            print()
        name, n, regs, mvr, vr = table(lines, sym, body0, region)
        print("== %s" % tag)
        show(name, n, regs, mvr, vr)


if __name__ == "__main__":
    main()
