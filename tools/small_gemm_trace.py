"""gemm_small launches of the joint step by their place in the step, from a rocprofv3 --kernel-trace csv (steps delimited by the adam kernel).
Launches are grouped by (template arguments, workgroups) and numbered in start order inside a step; decoder_exec.hip's sequence is fixed, so the
n-th launch of a group is the same projection in every step.  Average / min / max us per place over the second half of the steps, and per
K class for the two groups whose places differ in K (M x 512 outputs: 8 x ceil(M / 64) workgroups):
    NT, no activation: per layer  fc_s (K 512), q_c (512), fc_c (512), w_2 (1024)
    TB, no activation: head input gradient (4232), then per layer  w_1 (1024), fc_c (512), q_c (512), fc_s (512), Q|K|V (1536)
python tools/small_gemm_trace.py kernel_trace.csv [layers] > table.txt"""
import csv, sys, re, collections
rows = list(csv.DictReader(open(sys.argv[1])))
LAYERS = int(sys.argv[2]) if len(sys.argv) > 2 else 6
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
ends = [i for i, r in enumerate(rows) if "adam_kernel" in r["Kernel_Name"]]
first = len(ends) // 2
place = collections.defaultdict(list)      # (group, ordinal) -> durations
for s in range(first, len(ends) - 1):
    seen = collections.Counter()
    for r in rows[ends[s] + 1: ends[s + 1] + 1]:
        m = re.search(r"gemm_small_kernel<(\w+), (\d+)>", r["Kernel_Name"])
        if not m: continue
        wgs = int(r["Grid_Size"]) // int(r["Workgroup_Size"]) if "Workgroup_Size" in r else int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
        g = ("TB" if m.group(1) in ("true", "1") else "NT", int(m.group(2)), wgs)
        place[(g, seen[g])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        seen[g] += 1
groups = collections.defaultdict(list)
for (g, o), v in place.items(): groups[g].append((o, v))
NT_K = [512, 512, 512, 1024]
TB_K = [1024, 512, 512, 512, 1536]
byk = collections.defaultdict(list)
print(f"steps {first} .. {len(ends) - 2}; per place: launches, average / min / max us")
for g in sorted(groups):
    pl = sorted(groups[g])
    tot = sum(sum(v) / len(v) for _, v in pl)
    print(f"{g[0]} act={g[1]} workgroups={g[2]}: {len(pl)} launches per step, {tot:.1f} us per step")
    for o, v in pl:
        k = None
        if g[1] == 0 and len(pl) == 4 * LAYERS and g[0] == "NT": k = NT_K[o % 4]
        if g[1] == 0 and len(pl) == 5 * LAYERS + 1 and g[0] == "TB": k = 4232 if o == 0 else TB_K[(o - 1) % 5]
        if k: byk[(g[0], k)].extend(v)
        print(f"   {o:3d} {'K=%-5d' % k if k else '       '} n={len(v):4d}  {sum(v) / len(v):7.2f} {min(v):7.2f} {max(v):7.2f}")
print("by K (groups above whose places differ in K): launches, average us, median us")
for (tb, k), v in sorted(byk.items()):
    v = sorted(v)
    print(f"   {tb} K={k:5d}  n={len(v):5d}  {sum(v) / len(v):7.2f}  {v[len(v) // 2]:7.2f}")
