"""Static instruction counts of the per-row code of the k <= 64 solve kernel.

    hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -std=c++17 -fno-gpu-rdc \
        lkpy_amd/csrc/als_chol.hip -o als_chol.s
    python tools/factor_static_counts.py als_chol.s [more.s ...]

Reads the headline instantiation als_solve_kernel<4, false, false, false, false, true, false> and
counts, from the first panel's extraction to the row's store, the instructions by part and class.
The parts are told apart by what the instructions are, not by where the compiler put them:

  E  extraction: the basic blocks that hold a ds_write_b128 or the panel's ds_read_b128, the
     `v_mov_b32 v, 0` of the zeroed quad and the compares that are no column mask
  C  transposition: v_permlane*_swap and the s_nop in front of each
  U  update: v_mfma and the `v_xor_b32 0x80000000` negations
  F  the columns: everything else up to the last pivot's column
  B  back substitution and the row's epilogue: from the read of the reciprocal pivots on
"""
import collections
import re
import sys

KERNEL = "_ZN2lk16als_solve_kernelILi4ELb0ELb0ELb0ELb0ELb1ELb0EEE"
CLASSES = ("VALU", "cross-lane", "LDS", "MFMA", "scalar", "s_nop", "branch", "waitcnt", "VMEM")


def classify(op):
    if op.startswith("v_mfma"):
        return "MFMA"
    if op.startswith(("v_readlane", "v_readfirstlane", "v_permlane", "v_writelane")):
        return "cross-lane"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "VMEM"
    if op == "s_nop":
        return "s_nop"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op == "s_waitcnt":
        return "waitcnt"
    return "scalar"


def kernel_blocks(path):
    "the kernel's basic blocks: lists of (opcode, operands)"
    lines = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if ln.startswith(KERNEL) and re.match(r"^\S+:", ln))
    blocks, cur = [], []
    for ln in lines[start + 1:]:
        if ln.startswith(".Lfunc_end"):
            break
        if re.match(r"^\.LBB\S+:", ln) or ln.startswith("; %bb."):
            blocks.append(cur)
            cur = []
            continue
        m = re.match(r"^\t([a-z]\S*)\s*(.*)$", ln)
        if m and not m.group(1).startswith("."):
            cur.append((m.group(1), m.group(2)))
    blocks.append(cur)
    return [b for b in blocks if b]


def count(path):
    blocks = kernel_blocks(path)
    flat = [(bi, op, args) for bi, b in enumerate(blocks) for op, args in b]
    rsq = [i for i, (_, op, _) in enumerate(flat) if op.startswith("v_rsq")]
    assert len(rsq) == 64, len(rsq)
    e_blocks = {bi for bi, b in enumerate(blocks)
                if any(op in ("ds_write_b128", "ds_read_b128") for op, _ in b)}
    # the region starts with the first extraction block in front of the first pivot
    first = max(i for i, (bi, op, _) in enumerate(flat[:rsq[0]]) if op == "ds_write_b128")
    first = next(i for i, (bi, _, _) in enumerate(flat) if bi == flat[first][0])
    # ... and the back substitution with the read of the reciprocal pivots behind the last one
    back = next(i for i in range(rsq[-1], len(flat)) if flat[i][1] == "ds_read_b32")
    table = collections.defaultdict(collections.Counter)
    prev_nop = None
    for i in range(first, len(flat)):
        bi, op, args = flat[i]
        cls = classify(op)
        if i >= back:
            part = "B"
        elif op.startswith("v_permlane"):
            part = "C"
            if prev_nop is not None:  # the swap's own wait states
                table[prev_nop]["s_nop"] -= 1
                table["C"]["s_nop"] += 1
        elif cls == "MFMA" or (op.startswith("v_xor_b32") and "0x80000000" in args):
            part = "U"
        elif bi in e_blocks and blocks[bi][0][0] != "s_or_b64" and len(blocks[bi]) < 12:
            part = "E"
        elif op.startswith("v_mov_b32") and args.endswith(", 0"):
            part = "E"
        elif op.startswith("v_cmp") and not re.match(r"^(s\[\d+:\d+\]|vcc), \d+, v\d+$", args):
            part = "E"
        elif op in ("ds_write_b128", "ds_read_b128"):
            part = "E"
        else:
            part = "F"
        table[part][cls] += 1
        prev_nop = part if op == "s_nop" else None
    whole = collections.Counter(classify(op) for _, op, _ in flat)
    return table, whole, len(flat)


def main():
    for path in sys.argv[1:]:
        table, whole, n = count(path)
        print(f"# {path}")
        print(f"{'part':<6}" + "".join(f"{c:>11}" for c in CLASSES) + f"{'vector':>9}")
        total = collections.Counter()
        for part in "EFCUB":
            row = table[part]
            total.update(row)
            print(f"{part:<6}" + "".join(f"{row[c]:>11}" for c in CLASSES)
                  + f"{row['VALU'] + row['cross-lane']:>9}")
        print(f"{'sum':<6}" + "".join(f"{total[c]:>11}" for c in CLASSES)
              + f"{total['VALU'] + total['cross-lane']:>9}")
        print(f"{'kernel':<6}" + "".join(f"{whole[c]:>11}" for c in CLASSES)
              + f"{whole['VALU'] + whole['cross-lane']:>9}   ({n} instructions)")
        print()


if __name__ == "__main__":
    main()
