"""tools/isa_waits.py KERNEL.s SYMBOL [--cfg] -- the vector-memory instructions
and the s_waitcnt of a kernel's main loop, in program order, each with the
source line it came from (.loc; through inlined-at chains the outermost line
too).  SYMBOL is a substring of the kernel's mangled name that selects one
function (e.g. ImLi64ELb1ELb0ELb1ELi150E for k_mam_sm<unsigned long, 64, true,
false, true, 150>).  The main loop is the depth-1 loop of the function that
spans the most lines.  --cfg adds every block label and branch, to follow
which waits lie on which path.

What to read off it: whether an iteration's gathers are issued back to back
(no s_waitcnt with a vmcnt between them), whether a vmcnt wait stands between
the loop header and the first gather, and whether the loads are global_ or
flat_ (a flat load counts in lgkmcnt as well as vmcnt).  The .s comes from

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Iinclude --cuda-device-only \\
          -S -g1 smash-paper_amd/csrc/mam.hip

The footer repeats the kernel's register and spill counts from its metadata
comments.  Diagnostic tooling, like isa_regions.py."""
import re
import sys

VMEM = re.compile(r"^(global|flat|buffer|scratch)_(load|store|atomic)")


def function_lines(lines, sym):
    heads = [i for i, l in enumerate(lines)
             if re.match(r"^[A-Za-z_.$][\w.$]*:", l) and not l.startswith(".L") and sym in l.split(":")[0]]
    if len(heads) != 1:
        names = [lines[i].split(":")[0] for i in heads]
        sys.exit("SYMBOL must select one function; it selects %d: %s" % (len(heads), names[:8]))
    a = heads[0]
    b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return a, b


def main_loop(lines, a, b):
    """(header index, index of the last line) of the depth-1 loop that spans
    the most lines, by the block annotations the compiler writes ("in Loop:
    Header=BBn_m Depth=1", "Parent Loop BBn_m Depth=1")"""
    labels = [i for i in range(a, b) if re.match(r"^\.LBB\d+_\d+:", lines[i])] + [b]
    best = None
    for k, i in enumerate(labels[:-1]):
        m = re.match(r"^\.(LBB\d+_\d+):.*Loop Header: Depth=1", lines[i])
        if not m:
            continue
        tag = re.compile(r"(Header=|Parent Loop )%s Depth=1\b" % re.escape(m.group(1)[1:]))
        last = k
        for q in range(k + 1, len(labels) - 1):
            if any(tag.search(x) for x in lines[labels[q]:labels[q] + 3]):
                last = q
        end = labels[last + 1] - 1
        if best is None or end - i > best[1] - best[0]:
            best = (i, end)
    if best is None:
        sys.exit("no loop found")
    return best


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    cfg = "--cfg" in sys.argv
    if len(args) != 2:
        sys.exit(__doc__)
    lines = open(args[0]).read().split("\n")
    a, b = function_lines(lines, args[1])
    h, e = main_loop(lines, a, b)
    print("%s" % lines[a].split(":")[0])
    print("main loop: .s lines %d-%d (%d instructions)" % (
        h + 1, e + 1, sum(1 for l in lines[h:e + 1] if re.match(r"^\t[a-z]", l))))
    loc = ""
    n = {"vmem": 0, "flat": 0, "wait": 0, "vmwait": 0}
    pending_label = None
    for i in range(h, e + 1):
        l = lines[i]
        if "\t.loc\t" in l:
            chain = re.findall(r"([\w.]+):(\d+):\d+", l.split(";", 1)[1] if ";" in l else "")
            if chain:
                loc = "%s:%s" % chain[0]
                if len(chain) > 1 and chain[-1] != chain[0]:
                    loc += " < %s:%s" % chain[-1]
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            pending_label = m.group(1) + (" (loop header)" if i == h else "")
            if cfg:
                print("%s:" % pending_label)
                pending_label = None
            continue
        t = l.strip()
        if not re.match(r"^[a-z]", t):
            continue
        ins = t.split(";")[0].strip()
        op = ins.split()[0]
        show = False
        if VMEM.match(op):
            show = True
            n["vmem"] += 1
            n["flat"] += op.startswith("flat_")
        elif op == "s_waitcnt":
            show = True
            n["wait"] += 1
            n["vmwait"] += "vmcnt" in ins
        elif cfg and (op.startswith("s_cbranch") or op == "s_branch"):
            show = True
        if show:
            if pending_label:
                print("%s:" % pending_label)
                pending_label = None
            print("  %6d  %-58s %s" % (i + 1, ins, loc))
    print("loop: %d vector-memory instructions (%d flat), %d s_waitcnt (%d with vmcnt)" % (
        n["vmem"], n["flat"], n["wait"], n["vmwait"]))
    all_wait = sum(1 for l in lines[a:b] if l.strip().startswith("s_waitcnt"))
    all_ins = sum(1 for l in lines[a:b] if re.match(r"^\t[a-z]", l))
    all_valu = sum(1 for l in lines[a:b] if re.match(r"^\tv_", l))
    print("kernel: %d instructions, %d VALU, %d s_waitcnt" % (all_ins, all_valu, all_wait))
    name = lines[a].split(":")[0]
    info = next((i for i in range(b, len(lines)) if lines[i].startswith("; Kernel info:")), None)
    got = []
    for l in (lines[info:info + 20] if info is not None else []):
        m = re.match(r"^; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", l)
        if m:
            got.append("%s %s" % m.groups())
    # the spill counts stand in the code object's metadata, under the kernel's .name
    # (one "  - .key:" entry per kernel)
    md = next((i for i, l in enumerate(lines)
               if re.match(r"^\s+\.name:\s+%s$" % re.escape(name), l)), None)
    if md is not None:
        entry = re.compile(r"^  - \.")
        k0 = next(j for j in range(md, 0, -1) if entry.match(lines[j]))
        k1 = next((j for j in range(md + 1, len(lines))
                   if entry.match(lines[j]) or not lines[j].startswith(" ")), len(lines))
        for l in lines[k0:k1]:
            m = re.match(r"^\s+(?:- )?\.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)", l)
            if m:
                got.append("%s %s" % m.groups())
    print("kernel: " + ", ".join(got))


if __name__ == "__main__":
    main()
