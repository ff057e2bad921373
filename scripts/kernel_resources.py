"""Compact register / spill / LDS / occupancy table of one csrc/*.hip translation unit, compiled with the flags the library
is built with (build.CFLAGS and the unit's build.FILE_FLAGS; hipcc -Rpass-analysis=kernel-resource-usage):
    python scripts/kernel_resources.py conv_halo [substring of the demangled kernel name] [--isa]
--isa: also the number of v_mfma instructions and of all instructions of every kernel, counted in the unit's gfx950
assembly (--save-temps).
"lds" is the compiler's static LDS of the kernel; a kernel that takes its LDS dynamically at launch (extern __shared__: the
MLP, attention and most convolution kernels) shows 0 here, and its size is what the unit's *_lds_bytes function returns."""
import glob
import os
import re
import subprocess
import sys
import tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(root, "minkowskiengine_amd"))
import build  # noqa: E402  (the recipe only: importing the package would build and load the library)

args = [a for a in sys.argv[1:] if a != "--isa"]
isa = "--isa" in sys.argv
unit = args[0]
pat = args[1] if len(args) > 1 else ""


def demangle(name):
    # binutils' c++filt does not know DF16b; the vendor-extended spelling of the same type demangles to __bf16
    return subprocess.run(["c++filt", name.replace("DF16b", "u6__bf16")], capture_output=True, text=True).stdout.strip().split("(")[0]


with tempfile.TemporaryDirectory() as tmp:
    cmd = [build.HIPCC] + build.CFLAGS + build.FILE_FLAGS.get(unit + ".hip", []) + \
          os.environ.get("ME_AMD_EXTRA_HIPCC_FLAGS", "").split() + (["--save-temps"] if isa else []) + \
          ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, unit + ".hip"), "-o", os.path.join(tmp, unit + ".o")]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp).stderr
    # kernel -> [v_mfma, instructions].  Every global label opens an entry, kernel or not; only the entries whose name is
    # a kernel of the remarks are read below, and a kernel's text ends at .Lfunc_end before the next label
    counts, cur = {}, None
    for path in glob.glob(os.path.join(tmp, "*gfx950*.s")):
        for line in open(path):
            m = re.match(r"(\w+):\s", line)
            if m:
                cur = counts.setdefault(demangle(m.group(1)), [0, 0])
            elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and re.match(r"\t[a-z]\w+", line):
                cur[0] += line.startswith("\tv_mfma")
                cur[1] += 1
rows, cur = [], None
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"name": demangle(m.group(1))}
        rows.append(cur)
        continue
    m = re.search(r"([A-Za-z][A-Za-z \[\]/]*): (\S+) \[-Rpass-analysis", line)
    if m and cur is not None:
        cur[m.group(1)] = m.group(2)
for r in rows:
    if pat in r["name"]:
        tail = " mfma %d instr %d" % tuple(counts.get(r["name"], (-1, -1))) if isa else ""
        print("%-72s vgpr %s agpr %s sgpr %s sgpr-spill %s vgpr-spill %s scratch %s lds %s occ %s%s" % (
            r["name"][:72], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("SGPRs Spill"), r.get("VGPRs Spill"),
            r.get("ScratchSize [bytes/lane]"), r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]"), tail))
