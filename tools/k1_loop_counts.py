"""Static instruction counts of the K1 pair loops and the resources of every K1 kernel (no GPU needed).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -S --cuda-device-only tsu-emulator_amd/csrc/ising2d_tiled.hip -o tiled.s
    python tools/k1_loop_counts.py tiled.s [--before parent.s] [kernel-name-substring ...]

First a table of every k1_* kernel in the file: VGPRs, scratch bytes and occupancy as the compiler reports them (with --before:
beside the same figures of another build, regressions marked; a kernel whose template gained a trailing bool parameter since then is
compared with the other build's kernel of the name without it).  Then, for every kernel whose mangled name contains one of the
substrings (default: the two flagship tile-resident kernels), the VALU mnemonic histogram of every pair loop.

A pair loop is a loop (a label and the last backward branch to it or to a label just behind it) that holds LDS reads and at least
16 Philox multiplies and no other such loop.  Its hot path is counted: basic blocks that call the out-of-line tie path or belong to
the call's lane loop (s_swappc_b64, s_getpc_b64, v_readlane_b32, v_readfirstlane_b32) and the EDGE block of the wave-iteration that
straddles the wrap row (v_cndmask_b32 without an LDS access; one execution per half-sweep) are left out.  Forms are told apart by what only
they hold: EDGE by the scalar select of the row offset, SEAM by its 64-bit shifts (byte planes) or its extra masks (nibble
planes: at least 9 v_and_b32)."""
import collections
import re
import sys

DEFAULT = ["11k1_residentILi128ELi32ELi1024ELi1ELb0ELb0E", "11k1_residentILi512ELi32ELi1024ELi4ELb0ELb1E"]
COLD = ("s_swappc_b64", "s_getpc_b64", "v_readlane_b32", "v_readfirstlane_b32")


def kernels(path):
    name, out = None, {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name:
            out[name].append(line.rstrip("\n"))
            if line.startswith("; Occupancy"):
                name = None
    return out


def resources(body):
    text = "\n".join(body)
    return {k: int((re.search(r"; " + k + r":? =? ?(\d+)", text) or [None, "-1"])[1]) for k in ("NumVgprs", "ScratchSize", "Occupancy", "codeLenInByte")}


def mnemonics(lines):
    return collections.Counter(l.split()[0] for l in lines if re.match(r"^\t[a-z]", l))


def pair_loops(body):
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    by_end = {}
    for i, l in enumerate(body):
        m = re.match(r"^\ts_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            by_end[i] = min(by_end.get(i, i), labels[m.group(1)])
    # back edges that enter the same loop at neighbouring labels: one range from the first label to the last branch
    ranges = sorted((a, b) for b, a in by_end.items())
    merged = []
    for a, b in ranges:
        if merged and a <= merged[-1][1] and not (a > merged[-1][0] and b < merged[-1][1]):
            merged[-1] = (merged[-1][0], max(b, merged[-1][1]))
        else:
            merged.append((a, b))
    hot = []
    for a, b in merged:
        h = mnemonics(body[a:b + 1])
        if h.get("v_mad_u64_u32", 0) >= 16 and any(k.startswith("ds_read") for k in h):
            hot.append((a, b))
    return [r for r in hot if not any(o != r and r[0] <= o[0] and o[1] <= r[1] for o in hot)]


def hot_path(body, a, b):
    blocks, cur = [], []
    for l in body[a:b + 1]:
        if re.match(r"^\.LBB", l) and cur:
            blocks.append(cur)
            cur = []
        cur.append(l)
    blocks.append(cur)
    total = collections.Counter()
    for blk in blocks:
        h = mnemonics(blk)
        if any(k in h for k in COLD) or (h.get("v_cndmask_b32_e32") and not any(k.startswith("ds_") for k in h)):
            continue
        total += h
    return total


def main():
    args = sys.argv[1:]
    before = None
    if "--before" in args:
        i = args.index("--before")
        before = kernels(args[i + 1])
        del args[i:i + 2]
    body_of = kernels(args[0])
    print("every K1 kernel: VGPRs, scratch bytes, occupancy" + (" (before -> after)" if before else ""))
    for name, body in body_of.items():
        if "k1_" not in name:
            continue
        r = resources(body)
        # a kernel template that gained a trailing bool parameter: compare with the build before under the name without it
        was = name if not before or name in before else re.sub(r"Lb[01]E(Ev)", r"\1", name, count=1)
        if before and was in before:
            p = resources(before[was])
            worse = r["ScratchSize"] > p["ScratchSize"] or r["Occupancy"] < p["Occupancy"]
            print(f"  {name:78s} {p['NumVgprs']:3d} -> {r['NumVgprs']:3d}   {p['ScratchSize']:2d} -> {r['ScratchSize']:2d}   {p['Occupancy']} -> {r['Occupancy']}"
                  + ("   worse" if worse else ""))
        else:
            print(f"  {name:78s} {r['NumVgprs']:3d}   {r['ScratchSize']:2d}   {r['Occupancy']}")
    for want in args[1:] or DEFAULT:
        for name, body in body_of.items():
            if want not in name:
                continue
            r = resources(body)
            print(f"\n{name}\n  VGPRs {r['NumVgprs']}, scratch {r['ScratchSize']} bytes, occupancy {r['Occupancy']}, code {r['codeLenInByte']} bytes")
            for a, b in pair_loops(body):
                h = hot_path(body, a, b)
                if not h.get("v_mad_u64_u32"):  # a range made of cold blocks only (the lane loop of the tie call between two back edges)
                    continue
                valu = sorted(((k, v) for k, v in h.items() if k.startswith("v_")), key=lambda kv: (-kv[1], kv[0]))
                seam = h.get("v_lshrrev_b64") or h.get("v_and_b32_e32", 0) >= 9
                form = "SEAM" if seam else ("EDGE" if h.get("s_cselect_b32") else "plain")
                print(f"  {form:5s} loop, lines {a}-{b} of the kernel: {sum(v for _, v in valu)} VALU, "
                      f"{sum(v for k, v in h.items() if k.startswith('ds_read'))} LDS reads, {sum(v for k, v in h.items() if k.startswith('ds_write'))} LDS writes, "
                      f"{sum(v for k, v in h.items() if k.startswith('s_') and k not in ('s_nop', 's_waitcnt'))} scalar")
                print("        " + ", ".join(f"{k} {v}" for k, v in valu))


if __name__ == "__main__":
    main()
