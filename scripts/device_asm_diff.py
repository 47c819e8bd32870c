"""Per-kernel diff of two `hipcc -S --cuda-device-only` outputs: device_asm_diff.py PARENT.s NEW.s

For a refactor of a kernel source that must leave the device code alone. Each file is split at the
`Begin function` / `End function` markers; the function index in local labels (and in the comments that name
them: it moves with the order of instantiation) is normalised and whitespace collapsed. Per kernel: identical, or differing with the four resource fields of its descriptor and whether the
row kernels' loop -- from the first marked ring wait (`s_waitcnt vmcnt(K) expcnt(6)`) to the exit marker
(`... expcnt(5)`), register numbers masked -- is the same line for line. Exit status 1 when a kernel differs
or exists on one side only.
"""
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    """name -> normalised lines, from the Begin marker to the end of the kernel descriptor."""
    out, name = {}, None
    for line in open(path):
        m = re.search(r"-- Begin function (\S+)", line)
        if m:
            name, out[m.group(1)] = m.group(1), []
        if name is None:
            continue
        line = re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1N", " ".join(line.split()))
        line = re.sub(r"\bBB\d+_", "BBN_", line)  # the same index in the loop comments (Header=BB12_3)
        if line:
            out[name].append(line)
        if ".end_amdhsa_kernel" in line:
            name = None
    return out


def fields(lines):
    text = "\n".join(lines)
    return {f: int(m.group(1)) if (m := re.search(rf"\.amdhsa_{f} (\d+)", text)) else None for f in FIELDS}


def masked_loop(lines):
    """The instructions from the first ring wait to the exit marker, register numbers masked; None without both.
    Where the exit marker's block is laid out ahead of the loop (k_wgrad_rows): from it to the last s_endpgm."""
    code = [re.sub(r";.*", "", l).strip() for l in lines]
    first = next((i for i, l in enumerate(code) if re.match(r"s_waitcnt vmcnt\(\d+\) expcnt\(6\)", l)), None)
    last = next((i for i, l in enumerate(code) if "expcnt(5)" in l), None)
    if first is None or last is None:
        return None
    if last < first:
        first, last = last, max(i for i, l in enumerate(code) if l == "s_endpgm")
    return [re.sub(r"\b([asv])(\d+|\[\d+:\d+\])", r"\1#", l) for l in code[first:last + 1] if l]


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    differ = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            differ += 1
            print(f"ONLY IN {'PARENT' if name in a else 'NEW'}: {name}")
        elif a[name] != b[name]:
            differ += 1
            fa, fb, la, lb = fields(a[name]), fields(b[name]), masked_loop(a[name]), masked_loop(b[name])
            loop = "no ring markers" if la is None or lb is None else "same" if la == lb else "DIFFERS"
            print(f"DIFFERS: {name}")
            for f in FIELDS:
                print(f"    {f}: {fa[f]} -> {fb[f]}{'' if fa[f] == fb[f] else '   <-- changed'}")
            print(f"    masked loop (ring wait to exit marker): {loop}")
    print(f"{len(a)} kernels in parent, {len(b)} in new, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
