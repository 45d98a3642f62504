"""Static instruction counts per loop body of one kernel in a hipcc -S listing.

    python scripts/isa_loops.py k.s [KERNEL_SUBSTRING]

KERNEL_SUBSTRING picks the function (default: the headline kernel, k_tile<FS_PHONG, 4, false, MODE 2>).
Every backward branch is reported as a loop: the basic blocks from its target to the branch, with the
instructions in them by class (VALU, SALU, LDS, vector memory, scalar memory).  Nested loops are
reported on their own and again inside the loops that contain them; a body's count is static, taken
and untaken paths alike.
"""
import collections
import re
import sys

KERNEL = "k_tileILi1ELi4ELb0ELi2EE"


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    return "vmem"


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else KERNEL
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if want in l and l.endswith(":") is False and re.match(r"^_Z\S+:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], None
    for i, l in enumerate(lines[start:end]):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            cur = [m.group(1), i, []]
            blocks.append(cur)
            continue
        if cur is None:
            cur = ["entry", i, []]
            blocks.append(cur)
        s = l.strip()
        if re.match(r"^[vsdgb][a-z_0-9]+", s):
            cur[2].append(s)
    idx = {b[0]: k for k, b in enumerate(blocks)}
    tot = collections.Counter(classify(s.split()[0]) for b in blocks for s in b[2])
    print("%s: %d static instructions %s" % (lines[start].split(":")[0], sum(tot.values()), dict(tot)))
    for k, b in enumerate(blocks):
        for s in b[2]:
            m = re.match(r"s_(cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", s)
            if m and m.group(2) in idx and idx[m.group(2)] <= k:
                t = idx[m.group(2)]
                ins = [x.split()[0] for bb in blocks[t:k + 1] for x in bb[2]]
                c = collections.Counter(classify(x) for x in ins)
                rl = sum(1 for x in ins if x.startswith("v_readlane") or x.startswith("v_readfirstlane"))
                print("loop %s..%s (listing lines +%d..+%d): %4d instr  valu %4d (readlane %d)  salu %4d  lds %3d  vmem %3d  smem %3d"
                      % (blocks[t][0], b[0], blocks[t][1], b[1], len(ins), c["valu"], rl, c["salu"], c["lds"], c["vmem"], c["smem"]))


if __name__ == "__main__":
    main()
