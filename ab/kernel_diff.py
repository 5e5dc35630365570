"""Kernel-by-kernel comparison of two `hipcc -S --cuda-device-only` outputs of one unit, and the resource table of a
`-Rpass-analysis=kernel-resource-usage` log (profiles/hashgrid_batch_lod_disasm.txt, profiles/hashgrid_batch_lod_resources.txt).

    python ab/kernel_diff.py diff parent.s new.s [--commute] [--rename REGEX=REPLACEMENT ...]
    python ab/kernel_diff.py resources remarks.txt [name filter ...]

A kernel's text runs from its label to the end of its "Kernel info" comment block; its own mangled name, the function index of local labels
(.LBBn_ / BBn_) and of .Lfunc_endN, and runs of blanks are normalised.  Lines that name __hip_cuid are dropped.  --commute: a kernel that is
the parent's once the two source operands of its commutative two-operand instructions are put in one order - the same opcodes in the same order
on the same registers, the same resource block - is counted as "operands"  and the swapped lines are counted.  --rename: kernels
are paired by their demangled names; a parent's name goes through each re.sub(REGEX, REPLACEMENT) first, for a kernel that was renamed or
that became an instantiation of another template."""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*\)$", "", name)
    return name.replace("nic::hbatch::", "").replace("(bool)", "")


def kernels(path):
    """mangled name -> normalised text lines of every .amdhsa kernel of the file"""
    lines = open(path).read().splitlines()
    names = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    wanted = set(names)
    starts = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"(\S+):", ln)] if m and m.group(1) in wanted}
    out = {}
    for name in names:
        i = starts[name]
        j = i
        while not re.match(r"\s*\.end_amdhsa_kernel", lines[j]):
            j += 1
        body = []
        for ln in lines[i:j + 1]:
            if "__hip_cuid" in ln:
                continue
            ln = ln.replace(name, "KERNEL")
            ln = re.sub(r"\.?LBB\d+_", "LBB_", ln)
            ln = re.sub(r"\bBB\d+_", "BB_", ln)
            ln = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", ln)
            body.append(re.sub(r"\s+", " ", ln).strip())
        out[name] = body
    return out


COMMUTATIVE = re.compile(r"^([vs]_(?:xor|or|and|add_u32|mul_f32|add_f32|min|max)\w*) ([^,]+), ([^,]+), ([^,]+)$")


def commuted(ln):
    """the line with the two source operands of a commutative two-operand instruction sorted"""
    m = COMMUTATIVE.match(ln)
    if not m or m.group(1).startswith(("v_add_u32_sdwa", "v_mul_f32_sdwa")) or "dpp" in m.group(1):
        return ln
    x, y = sorted((m.group(3), m.group(4)))
    return f"{m.group(1)} {m.group(2)}, {x}, {y}"


def diff(parent, new, commute=False, renames=()):
    a, b = kernels(parent), kernels(new)
    names = demangle(sorted(set(a) | set(b)))

    def was(n):                                             # the parent's kernel under the name it has now
        for pattern, repl in renames:
            n = re.sub(pattern, repl, n)
        return n
    a = {was(short(names[m])): body for m, body in a.items()}
    b = {short(names[m]): body for m, body in b.items()}
    same = moved = swapped = swapped_lines = 0
    rows = []
    for n in sorted(set(a) | set(b)):
        if n not in a:
            rows.append(f"new       {'':>7} {len(b[n]):>7}  {n}")
        elif n not in b:
            rows.append(f"GONE      {len(a[n]):>7} {'':>7}  {n}")
        elif a[n] == b[n]:
            same += 1
            rows.append(f"identical {len(a[n]):>7} {len(b[n]):>7}  {n}")
        elif commute and len(a[n]) == len(b[n]) and [commuted(ln) for ln in a[n]] == [commuted(ln) for ln in b[n]]:
            k = sum(x != y for x, y in zip(a[n], b[n]))
            swapped += 1
            swapped_lines += k
            rows.append(f"operands  {len(a[n]):>7} {len(b[n]):>7}  {n}  ({k} line{'s' if k > 1 else ''})")
        else:
            moved += 1
            rows.append(f"DIFFERENT {len(a[n]):>7} {len(b[n]):>7}  {n}")
    print(f"{len(a)} kernels at the parent, {len(b)} now; of the parent's: identical {same}, "
          + (f"operand order only {swapped} ({swapped_lines} lines), " if commute else "")
          + f"different {moved}, gone {len(set(a) - set(b))}; new {len(set(b) - set(a))}")
    print("\n".join(rows))
    return moved + len(set(a) - set(b))


def resources(path, filters):
    keys = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]
    recs, cur = [], None
    for ln in open(path):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", ln)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            recs.append(cur)
        elif cur is not None:
            for k in keys:
                if t.startswith(k + ":"):
                    cur[k] = t.split(":", 1)[1].strip()
    names = demangle([r["name"] for r in recs])
    print(f"{'kernel':<52}SGPRs VGPRs AGPRs scratch B/lane VGPR spill SGPR spill occupancy   LDS B")
    for r in sorted(recs, key=lambda r: names[r["name"]]):
        n = short(names[r["name"]])
        if filters and not any(f in n for f in filters):
            continue
        print(f"{n:<52}{r[keys[0]]:>5} {r[keys[1]]:>5} {r[keys[2]]:>5} {r[keys[3]]:>14} {r[keys[4]]:>10} {r[keys[5]]:>10} {r[keys[6]]:>9} {r[keys[7]]:>7}")


if __name__ == "__main__":
    if sys.argv[1] == "diff":
        rest = sys.argv[4:]
        renames = [tuple(rest[i + 1].split("=", 1)) for i, x in enumerate(rest) if x == "--rename"]
        sys.exit(1 if diff(sys.argv[2], sys.argv[3], "--commute" in rest, renames) else 0)
    resources(sys.argv[2], sys.argv[3:])
