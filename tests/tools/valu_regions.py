"""Lab tool: static instruction counts of inflate_kernel<11,false,false> between its PZG_MARK labels, the vector operations by
the cost classes of profiles/r04_op_cost.txt.  It compiles pzg_kernels.hip for gfx950 with -DPZG_MARKS to device assembly
(no GPU needed; the marks are assembly comments, so they exist in the compiler's assembly and not in a linked library -- the
options are read from the product's Makefile) and reads that.  It decides what to look at; it checks nothing.

    python tests/tools/valu_regions.py [--label NAME] [--src DIR] [--all] [extra compiler flags, e.g. -DPZG_SEQ_GROUP=4]

--src DIR: another checkout's pure_zlib_amd/csrc (the parent's, for the "before" table).  --all: every region, not only the
phases' (sa, sb, g.*).

The classes (SIMD cycles per wave-instruction, measured with 16 waves per CU):
  full  2.2   v_add/v_sub/v_and/v_or/v_xor/v_mov/v_lshrrev/v_ashrrev in the 32-bit encoding, registers and inline constants only
  mid   2.6   the same with a 32-bit literal, or in the 64-bit encoding without a scalar operand
  half  4.3   everything else: a scalar register operand (vcc and exec included), three operands, SDWA, DPP, v_cndmask, v_cmp,
              v_lshlrev, v_min/v_max, v_mul, v_readlane ...
`cyc` = 2.2 full + 2.6 mid + 4.3 half: the region's weighted vector cycles, once through in layout order.  A region is what lies
between a mark and the next one in the file's order: blocks the compiler moved elsewhere are counted where they landed."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = "/opt/rocm/bin/hipcc"


def product_flags():
    """the product's own compiler options for pzg_kernels.hip, read from its Makefile (HIPFLAGS and KERNELFLAGS: no copy to drift)"""
    var = {}
    for l in open(os.path.join(ROOT, "pure_zlib_amd", "csrc", "Makefile")):
        m = re.match(r"(\w+) := (.*)$", l)
        if m:
            var[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda x: var.get(x.group(1), ""), m.group(2)).strip()
    return [f for f in (var["HIPFLAGS"] + " " + var["KERNELFLAGS"]).split() if f not in ("-fPIC", "-Wall")]


KERNEL = "_ZN3pzg14inflate_kernelILi11ELb0ELb0EEEvNS_11InflateArgsE"
CHEAP = {"v_add_u32", "v_sub_u32", "v_subrev_u32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_mov_b32", "v_lshrrev_b32", "v_ashrrev_i32"}
COST = {"full": 2.2, "mid": 2.6, "half": 4.3}
PHASES = ("sa.begin", "sb.begin", "g.begin", "g.lits", "g.matches", "g.far", "g.rounds", "g.end")
INLINE_F = {"0.5", "-0.5", "1.0", "-1.0", "2.0", "-2.0", "4.0", "-4.0"}


def valu_class(op, operands):
    """the cost class of one vector instruction, from its assembly text"""
    m = re.match(r"(v_\w+?)(_e32|_e64|_sdwa|_dpp|_e64_dpp)?$", op)
    base, enc = m.group(1), m.group(2) or ""
    if base not in CHEAP or enc in ("_sdwa", "_dpp", "_e64_dpp"):
        return "half"
    srcs = [x.strip() for x in operands.split(",")][1:]
    lit = False
    for s in srcs:
        if re.match(r"(s\d+|s\[|vcc|exec|m0|ttmp|src_|scc)", s):
            return "half"
        if re.match(r"v\d+|v\[", s):
            continue
        if s in INLINE_F:
            continue
        try:
            lit |= not -16 <= int(s, 0) <= 64
        except ValueError:
            lit = True  # (a symbol or an expression: encoded as a literal)
    return "mid" if lit or enc == "_e64" else "full"


def kernel_lines(asm):
    on = False
    for l in asm.splitlines():
        if l.startswith(KERNEL + ":"):
            on = True
        if on:
            yield l
            if l.startswith(".Lfunc_end"):
                return


def regions(asm):
    out, cur, c = [], "(start)", collections.Counter()
    for l in kernel_lines(asm):
        m = re.search(r"##MARK (\S+)", l)
        if m:
            out.append((cur, c))
            cur, c = m.group(1), collections.Counter()
            continue
        m = re.match(r"\s+([vs]_\w+|ds_\w+|global_\w+|buffer_\w+|flat_\w+|scratch_\w+)\s*(.*?)\s*(;.*)?$", l)
        if not m:
            continue
        op, operands = m.group(1), m.group(2)
        if op.startswith(("s_waitcnt", "s_nop")):
            c["wait"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("v_"):
            c[valu_class(op, operands)] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        else:
            c["vmem"] += 1
    out.append((cur, c))
    return out


def main(argv):
    label, src, every, extra = "", os.path.join(ROOT, "pure_zlib_amd", "csrc"), False, []
    it = iter(argv)
    for a in it:
        if a == "--label":
            label = next(it)
        elif a == "--src":
            src = os.path.abspath(next(it))
        elif a == "--all":
            every = True
        else:
            extra.append(a)
    out = os.path.join(ROOT, "build", "asm")
    os.makedirs(out, exist_ok=True)
    s = os.path.join(out, "valu_regions_%s.s" % (label or "tree"))
    subprocess.check_call([HIPCC] + product_flags() + ["--cuda-device-only", "-DPZG_MARKS", "-w"] + extra + ["-S", "pzg_kernels.hip", "-o", s], cwd=src)
    asm = open(s).read()
    notes = re.search(r"\.amdhsa_kernel " + KERNEL + r"(.*?)\.end_amdhsa_kernel", asm, re.S).group(1)
    regs = {k: int(v) for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size) (\d+)", notes)}
    print("# %s%s  inflate_kernel<11,false,false>: vgpr %d sgpr %d lds %d scratch %d" % (
        label or "tree", (" " + " ".join(extra)) if extra else "", regs["next_free_vgpr"], regs["next_free_sgpr"],
        regs["group_segment_fixed_size"], regs["private_segment_fixed_size"]))
    print("# a region = the lines between a mark and the next one in the file's order: it depends on where the compiler laid the blocks out")
    print("# (a row that changes by far more than the source did has other blocks between its marks; g.end is whatever follows a group).")
    print("# The kernel holds every phase once per copy of token_loop<> (fixed code, dynamic codes); g.begin..end sums the groups' regions of ALL copies.")
    print("%-12s %5s %5s %5s %5s %8s %5s %5s %5s %5s" % ("region", "valu", "full", "mid", "half", "cyc", "salu", "lds", "vmem", "wait"))
    tot = collections.Counter()
    for name, c in regions(asm):
        if not every and name not in PHASES:
            continue
        valu = c["full"] + c["mid"] + c["half"]
        cyc = sum(COST[k] * c[k] for k in COST)
        print("%-12s %5d %5d %5d %5d %8.1f %5d %5d %5d %5d" % (name, valu, c["full"], c["mid"], c["half"], cyc, c["salu"], c["lds"], c["vmem"], c["wait"]))
        key = "g.*" if name.startswith("g.") and name != "g.end" else None
        if key:
            tot.update(c)
    valu = tot["full"] + tot["mid"] + tot["half"]
    print("%-12s %5d %5d %5d %5d %8.1f %5d %5d %5d %5d" % ("g.begin..end", valu, tot["full"], tot["mid"], tot["half"], sum(COST[k] * tot[k] for k in COST),
                                                      tot["salu"], tot["lds"], tot["vmem"], tot["wait"]))


if __name__ == "__main__":
    main(sys.argv[1:])
