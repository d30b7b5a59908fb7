"""TN-only, many-arm version of tools/probes/mfma_shape_ab.py: arm A (first --lib) is the reference; one discarded round, then --rounds interleaved."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import mfma_shape_ab as ab

ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", required=True, help="name=path; first is arm A")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--json", default=None)
a = ap.parse_args()
torch.cuda.set_device(0)
names = [x.split("=")[0] for x in a.lib]
libs = {x.split("=")[0]: ab.load(x.split("=")[1]) for x in a.lib}
rows = [r for r in ab.table_rows(os.path.join(ROOT, "profiles", "r06_roofline_by_shape.md")) if r[0] != "gemm_nt" and ab.served(r[0], *r[2:5])]
print("arms:", names, len(rows), "rows", flush=True)
per = {}
for r in rows:
    entry, kind, M, N, K, calls = r
    call, hold = ab.make_call(entry, kind, M, N, K, list(libs.values()))
    for n in names:
        ab.timed(call, libs[n], 3)
    reps = max(3, int(40.0 / max(ab.timed(call, libs[names[0]], 3), 1e-3)))
    per[r] = {n: [] for n in names}
    for rd in range(-1, a.rounds):
        k = (rd + 1) % len(names)
        for n in names[k:] + names[:k]:
            t = ab.timed(call, libs[n], reps)
            if rd >= 0:
                per[r][n].append(t)
    md = {n: statistics.median(per[r][n]) for n in names}
    print(f"| {entry} | {kind} | [{M}, {N}, {K}] | {calls} | " + " | ".join(f"{md[n]:.4f}" for n in names) + " | " + " | ".join(f"{md[n] / md[names[0]]:.4f}" for n in names[1:]) + " |", flush=True)
    del call, hold
    torch.cuda.empty_cache()
sums = {n: [sum(r[5] * per[r][n][rd] for r in rows) for rd in range(a.rounds)] for n in names}
A = names[0]
spread = max(sums[A]) - min(sums[A])
for n in names:
    med = statistics.median(sums[n])
    gain = statistics.median(sums[A]) - med
    print(f"{n}: " + " ".join(f"{v:.3f}" for v in sums[n]) + f"  median {med:.3f}  A - this = {gain:+.3f} ms; 3 x spread of A = {3 * spread:.3f} -> {'WINS' if gain > 3 * spread else 'does not win'}")
if a.json:
    json.dump(dict(names=names, sums=sums, rows=[dict(entry=r[0], kind=r[1], shape=r[2:5], calls=r[5], **per[r]) for r in rows]), open(a.json, "w"))
