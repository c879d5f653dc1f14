#!/usr/bin/env python3
"""Per-kernel fingerprint of a HIP translation unit's device side, to show that a host-side change left the kernels alone.
  tools/kernel_table.py dump <source.hip> <out.json>        cross-compile the device side for gfx950 with the build's flags; per kernel symbol:
                                                            sha256 of its llvm-objdump -d text (addresses / comments / alignment padding stripped) + the resource notes
  tools/kernel_table.py compare <before.json> <after.json> <out.txt>      two-column table, one kernel per entry
Needs no GPU.  The LLVM tools are taken from $ROCM_PATH/llvm/bin (default /opt/rocm)."""
import hashlib, json, os, re, subprocess, sys, tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "phaser_amd", "csrc")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def dump(src, out):
    with tempfile.TemporaryDirectory() as td:
        obj = os.path.join(td, "dev.o")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(REPO, "include"), "-I" + CSRC,
                               "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj])
        dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", obj], text=True)
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], text=True)
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1); code[cur] = []
        elif cur is not None and line.strip() and line.strip() != "...":          # ("...": the zero padding up to the next symbol's alignment, not part of the kernel)
            code[cur].append(re.sub(r"\s*//.*$", "", line).strip())
    tab = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        f = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(\S+)\s*$", ".agpr_count:" + blk, re.M))
        name = f[".name"]
        tab[name] = {"sha": hashlib.sha256("\n".join(code[name]).encode()).hexdigest()[:16], **{k: f.get("." + k) for k in KEYS}}
    json.dump(tab, open(out, "w"), indent=1, sort_keys=True)
    print(len(tab), "kernels")


def compare(before, after, out):
    b, a = json.load(open(before)), json.load(open(after))
    fmt = lambda r: "-" if r is None else "%s v%s a%s s%s spill %s/%s lds %s scratch %s" % ((r["sha"],) + tuple(r[k] for k in KEYS))
    lines = ["per kernel symbol, device side cross-compiled for gfx950 with the build's flags (-O3 -std=c++17 -fPIC --cuda-device-only --no-gpu-bundle-output):",
             "sha256[:16] of the llvm-objdump -d text (addresses, comments and alignment padding stripped), then VGPRs, AGPRs, SGPRs, spills vgpr/sgpr, LDS bytes, scratch bytes from llvm-readelf --notes",
             "", "%-8s %s" % ("status", "symbol"), "         before | after", ""]
    changed = 0
    for k in sorted(set(a) | set(b)):
        fb, fa = fmt(b.get(k)), fmt(a.get(k))
        st = "same" if fb == fa else ("deleted" if k not in a else ("NEW" if k not in b else "DIFFERS"))
        changed += st in ("NEW", "DIFFERS")
        lines += ["%-8s %s" % (st, k), "         %s | %s" % (fb, fa)]
    lines += ["", "%d kernels before, %d after; deleted: %s; new or different: %d" % (len(b), len(a), ", ".join(sorted(set(b) - set(a))) or "none", changed)]
    open(out, "w").write("\n".join(lines) + "\n")
    print(lines[-1])
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4]))
    else:
        sys.exit(__doc__)
