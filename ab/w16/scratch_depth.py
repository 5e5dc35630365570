"""where the spills of fused_train16_kernel sit: for every instantiation in an assembly dump (ab/isa.sh flags + -fno-slp-vectorize, --cuda-device-only -S
of csrc/fused_t16.hip), the loop depth (the compiler's "in Loop: Header=.. Depth=N" block comments) of every scratch access and of the MFMAs.
Depth 0 = launch prologue / epilogue, 1 = segment loop, 2 = work-unit loop, 3 = the round loop.   python ab/w16/scratch_depth.py t16.s"""
import re, sys, collections
kern, depth = None, 0
acc, mfma = collections.defaultdict(list), collections.defaultdict(collections.Counter)
for l in open(sys.argv[1]):
    m = re.match(r"^(_ZN3nic\w+):", l)
    if m:
        kern, depth = (re.sub(r".*LayoutILi(\d)EEELi(\d).*", r"Layout<\1>, MODE \2", m.group(1)) if "fused_train16" in m.group(1) else None), 0
        continue
    if kern is None:
        continue
    if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
        d = re.search(r"Depth=(\d+)", l)
        depth = int(d.group(1)) if d else 0
    elif "scratch_" in l:
        acc[kern].append((depth, l.split()[0]))
    elif "v_mfma" in l:
        mfma[kern][depth] += 1
for k in mfma:
    print(f"{k}: MFMAs by depth {dict(mfma[k])}; scratch accesses by depth {dict(collections.Counter(d for d, _ in acc[k]))}"
          f"{'  <-- IN THE ROUND LOOP' if any(d >= 3 for d, _ in acc[k]) else ''}")
