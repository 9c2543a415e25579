"""Static report on the generated code of the library's kernels.

Compiles every csrc/*.hip (or the files named on the command line) to gfx950 assembly with
build.py's flags and prints, per kernel: code bytes, VGPRs, occupancy, scratch bytes, spilled
scalars, the number of lane moves (v_readlane_b32 / v_writelane_b32: scalar spill traffic),
the number of matrix-core instructions, how many of those directly follow a full LDS wait
(s_waitcnt lgkmcnt(0) as the previous instruction: an MFMA that waits for its own operands'
round trip), and the number of double-precision vector instructions (v_*_f64*: the chip has no
scalar double arithmetic, so uniform double math such as the Adam bias corrections' pow runs on
the vector unit; static count, taken or not), and the number of flat loads and stores (flat_load* /
flat_store*: accesses through a pointer whose address space the compiler does not know, which
count as a memory and an LDS access at once).  The assembly is read for these quantities only.

  python scripts/chain_report.py [--filter SUBSTR] [--csrc DIR] [--keep DIR] [file.hip ...]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "redcliff-s-hypothesizing-dynamic-causal-graphs_amd"))
from redcliff_amd import build as B  # noqa: E402

_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
_INFO = {
    "code": re.compile(r"^; codeLenInByte = (\d+)"),
    "occ": re.compile(r"^; Occupancy: (\d+)"),
    "scratch": re.compile(r"^; ScratchSize: (\d+)"),
}
_META_NAME = re.compile(r"^\s+\.name:\s+(\S+)")
_META_SPILL = re.compile(r"^\s+\.sgpr_spill_count:\s+(\d+)")
_META_VGPR = re.compile(r"^\s+\.vgpr_count:\s+(\d+)")
_FULL_LDS_WAIT = re.compile(r"^s_waitcnt\b.*lgkmcnt\(0\)")


def assemble(src, csrc, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=%s" % B.ARCH, "-O3", "-std=c++17", "-I" + B.INCLUDE, "-I" + csrc,
           '-DREDCLIFF_BUILD_ID="report"', "--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd)


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def parse(path):
    """{kernel symbol: counts} of one assembly file."""
    kernels, spills, vgprs = {}, {}, {}
    cur, prev, name = None, "", None
    with open(path) as f:
        lines = f.read().splitlines()
    for raw in lines:
        line = raw.strip()
        m = _META_NAME.match(raw)
        if m:
            name = m.group(1)
        m = _META_SPILL.match(raw)
        if m and name:
            spills[name] = int(m.group(1))
        m = _META_VGPR.match(raw)
        if m and name:
            vgprs[name] = int(m.group(1))
        m = _LABEL.match(raw)
        if m and not m.group(1).startswith(".L"):
            cur = {"lane": 0, "mfma": 0, "mfma_wait": 0, "f64": 0, "flat": 0}
            kernels[m.group(1)] = cur
            prev = ""
            continue
        if cur is None:
            continue
        done = False
        for key, rx in _INFO.items():
            m = rx.match(line)
            if m:
                cur[key] = int(m.group(1))
                done = True
        if done or not line or line[0] in ";." or _LABEL.match(line):
            continue
        op = line.split()[0]
        if op in ("v_readlane_b32", "v_writelane_b32"):
            cur["lane"] += 1
        elif op.startswith("v_mfma_"):
            cur["mfma"] += 1
            if _FULL_LDS_WAIT.match(prev):
                cur["mfma_wait"] += 1
        elif op.startswith("v_") and "_f64" in op:
            cur["f64"] += 1
        elif op.startswith(("flat_load", "flat_store")):
            cur["flat"] += 1
        prev = line
    out = {}
    for sym, k in kernels.items():
        if "code" in k and sym in spills:  # kernels only (they have a metadata entry)
            k["spill"] = spills[sym]
            k["vgpr"] = vgprs.get(sym, -1)
            out[sym] = k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="*")
    ap.add_argument("--csrc", default=B.CSRC, help="source directory (another tree's csrc to report on it)")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--keep", default="", help="write the assembly files into this directory")
    a = ap.parse_args()
    files = a.files or sorted(os.path.join(a.csrc, f) for f in os.listdir(a.csrc) if f.endswith(".hip"))
    print("%-58s %8s %5s %3s %7s %6s %6s %5s %9s %5s %5s" %
          ("kernel", "bytes", "vgpr", "occ", "scratch", "sspill", "lanemv", "mfma", "mfma@wait", "f64", "flat"))
    with tempfile.TemporaryDirectory(prefix="rc_asm_") as tmp:
        if a.keep:
            os.makedirs(a.keep, exist_ok=True)
        outs = [os.path.join(a.keep or tmp, os.path.basename(src) + ".s") for src in files]
        with ThreadPoolExecutor(max(1, min(len(files), int(os.environ.get("MAX_JOBS", os.cpu_count() or 4)), 16))) as ex:
            list(ex.map(lambda so: assemble(so[0], a.csrc, so[1]), zip(files, outs)))
        for src, out in zip(files, outs):
            ks = parse(out)
            names = demangle(list(ks))
            rows = sorted(((re.sub(r"^void |\(anonymous namespace\)::| \[clone.*$|\([^()]*\)$", "", names[s]), k) for s, k in ks.items()),
                          key=lambda r: r[0])
            rows = [r for r in rows if a.filter in r[0]]
            if rows:
                print("# %s" % os.path.basename(src))
            for nm, k in rows:
                print("%-58s %8d %5d %3d %7d %6d %6d %5d %9d %5d %5d" %
                      (nm[:58], k["code"], k.get("vgpr", -1), k.get("occ", -1), k.get("scratch", -1), k["spill"],
                       k["lane"], k["mfma"], k["mfma_wait"], k["f64"], k["flat"]))


if __name__ == "__main__":
    main()
