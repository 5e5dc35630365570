"""where the spills of fused_train16_kernel sit: for every instantiation in an assembly dump (ab/isa.sh flags + -fno-slp-vectorize, --cuda-device-only -S
of csrc/fused_t16.hip), the loop depth (the compiler's "in Loop: Header=.. Depth=N" block comments) of every scratch access and of the MFMAs.
Depth 0 = launch prologue / epilogue, 1 = segment loop, 2 = work-unit loop, 3 = the round loop (one less each where the compiler unrolled the two segments: the round loop is the depth with the 158 MFMAs).   python ab/w16/scratch_depth.py t16.s"""
import re, sys, collections
kern, depth = None, 0
acc, mfma = collections.defaultdict(list), collections.defaultdict(collections.Counter)
lines = open(sys.argv[1]).read().split("\n")
for i, l in enumerate(lines):
    m = re.match(r"^(_ZN3nic\w+):", l)
    if m:
        kern, depth = (re.sub(r".*LayoutILi(\d)EEELi(\d).*", r"Layout<\1>, MODE \2", m.group(1)) if "fused_train16" in m.group(1) else None), 0
        continue
    if kern is None:
        continue
    if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
        # the block's loop comment sits on the label's line or on the comment lines right after it; a nested header lists its parent loops first
        head = [l]
        for n in lines[i + 1:i + 12]:
            if not n.lstrip().startswith(";"):
                break
            head.append(n)
        own = [h for h in head if "Loop Header" in h] or [h for h in head if "in Loop:" in h]
        d = re.search(r"Depth=(\d+)", own[0]) if own else None
        depth = int(d.group(1)) if d else 0
    elif "scratch_" in l:
        acc[kern].append((depth, l.split()[0]))
    elif "v_mfma" in l:
        mfma[kern][depth] += 1
for k in mfma:
    rd = max(mfma[k], key=lambda d: mfma[k][d])        # the round loop: the depth that holds its MFMAs (3, or 2 where the compiler unrolled the two segments)
    print(f"{k}: MFMAs by depth {dict(mfma[k])}; scratch accesses by depth {dict(collections.Counter(d for d, _ in acc[k]))}"
          f"{'  <-- IN THE ROUND LOOP' if any(d >= rd for d, _ in acc[k]) else ''}")
