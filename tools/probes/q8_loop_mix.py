"""Instruction mix of the steady K tile of every gemm_nt_q8_kernel instantiation, read from the compiler's ISA (build host, no GPU).

    cd fiber_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value --cuda-device-only -S gemm.hip -o /tmp/gemm.s
    python tools/probes/q8_loop_mix.py /tmp/gemm.s [more.s ...]

The steady K tile is found, not named: among the loops of a kernel (a label and a later branch back to it) the shortest one whose steady path
holds exactly 64 MFMAs, 24 ds_read_b128 and 8 global_load_lds_dwordx4.  The steady path through a loop segment takes every forward branch whose
target lies inside the segment and that skips no MFMA, LDS read or DMA request (the end-of-tile code of the cursor is such a skipped range) and
falls through every other branch.  Counted on that path:
  SALU = s_* other than s_nop / s_waitcnt / s_barrier / s_setprio / branches / scalar memory (s_load*, s_memtime, s_memrealtime)
  VALU = v_* other than v_mfma*;   waits = s_waitcnt;   static = SALU of the whole segment, skipped ranges included."""
import re
import subprocess
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    out, i = [], 0
    while i < len(lines):
        m = re.match(r"^(_ZN\S*17gemm_nt_q8_kernelI\S+):", lines[i])
        if m:
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            out.append((m.group(1), [ln.split(";")[0].strip() for ln in lines[i + 1:j]]))
            i = j
        i += 1
    return out


def kind(t):
    op = t.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("ds_read"):
        return "ds_read"
    if op.startswith("global_load_lds"):
        return "dma"
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "waits"
    if op == "s_barrier":
        return "barriers"
    if op == "s_setprio":
        return "s_setprio"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branches"
    if op.startswith("s_load") or op.startswith("s_memtime") or op.startswith("s_memrealtime"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "valu"
    return "other"


def walk(body, lo, hi, label_at):
    """Counts on the steady path of body[lo:hi + 1]."""
    c, i = {}, lo
    while i <= hi:
        t = body[i]
        if not t or t.endswith(":") or t.startswith("."):
            i += 1
            continue
        k = kind(t)
        c[k] = c.get(k, 0) + 1
        if k == "branches" and i != hi:
            tgt = label_at.get(t.split()[-1])
            if tgt is not None and i < tgt <= hi:
                skipped = [kind(x) for x in body[i + 1:tgt] if x and not x.endswith(":") and not x.startswith(".")]
                if not any(s in ("mfma", "ds_read", "dma") for s in skipped):
                    i = tgt
                    continue
        i += 1
    return c


def steady(body):
    label_at = {t[:-1]: i for i, t in enumerate(body) if t.endswith(":")}
    best = None
    for i, t in enumerate(body):
        if t and kind(t) == "branches":
            lo = label_at.get(t.split()[-1])
            if lo is not None and lo < i:
                c = walk(body, lo, i, label_at)
                if (c.get("mfma"), c.get("ds_read"), c.get("dma")) == (64, 24, 8) and (best is None or i - lo < best[0]):
                    static = sum(1 for x in body[lo:i + 1] if x and not x.endswith(":") and not x.startswith(".") and kind(x) == "salu")
                    best = (i - lo, c, static)
    return best


def main():
    cols = ["salu", "valu", "s_nop", "s_setprio", "branches", "waits", "barriers", "smem", "mfma", "ds_read", "dma"]
    for path in sys.argv[1:]:
        print(f"\n{path}\n| instantiation | " + " | ".join(cols) + " | static SALU of the segment |\n|---|" + "---|" * (len(cols) + 1))
        ks = kernels(path)
        names = subprocess.run(["c++filt"], input="\n".join(k[0].replace("DF16b", "Dh") for k in ks), capture_output=True, text=True).stdout.splitlines()
        for (_, body), name in sorted(zip(ks, names), key=lambda p: p[1]):
            name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "").replace("void ", "")).replace("gemm_nt_q8_kernel", "")
            b = steady(body)
            if b is None:
                print(f"| {name} | no loop with a 64 / 24 / 8 steady path |")
            else:
                print(f"| {name} | " + " | ".join(str(b[1].get(c, 0)) for c in cols) + f" | {b[2]} |")


if __name__ == "__main__":
    main()
