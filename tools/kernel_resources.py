#!/usr/bin/env python3
"""Per-kernel resource usage of the gfx950 HIP kernels, from the compiler.

Compiles the given distributed_training_guide_amd/_hip/*.hip files (all of
them by default) for the device only, with the flags of tools/build_hip.py
plus -Rpass-analysis=kernel-resource-usage, and prints one row per kernel:
VGPRs, scratch bytes per lane, occupancy (waves per SIMD) and static LDS.
Needs hipcc, not a GPU.

Scratch is the column to watch: a kernel that should keep its state in
registers and reports scratch is reading and writing private memory behind
the source's back (a private array indexed by a run-time loop counter does
that), and no test of results can see it.

--loops additionally reads the ISA of each kernel that uses MFMA and counts,
inside its main loop (the tightest backward branch that encloses all of its
MFMAs; a static count, so the masked path of a tile counts with the rest):
MFMAs, branches, full LDS waits (s_waitcnt lgkmcnt(0)), counted LDS waits
and the vector instructions that are not MFMA.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
HIP_DIR = REPO / "distributed_training_guide_amd" / "_hip"
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")

_REMARK = re.compile(r"remark: (?:\s*)([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)")
_FIELDS = {
    "Function Name": "name",
    "VGPRs": "vgprs",
    "ScratchSize": "scratch",
    "Occupancy": "occupancy",
    "LDS Size": "lds",
}


def device_flags():
    """The build's flags that shape device code (tools/build_hip.py)."""
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-DUSE_ROCM=1",
             "-D__HIP_PLATFORM_AMD__=1", f"-I{HIP_DIR}"]
    if os.environ.get("DTGA_HIP_FLAGS"):
        flags += os.environ["DTGA_HIP_FLAGS"].split()
    return flags


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), text=True,
                             capture_output=True, check=True).stdout
        return [re.sub(r"\(.*", "", re.sub(r"^void ", "", n))
                for n in out.splitlines()]
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def parse_remarks(text):
    """Rows of {name, vgprs, scratch, occupancy, lds} from hipcc's remarks."""
    rows, cur = [], None
    for line in text.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        key = _FIELDS.get(m.group(1).strip())
        if key is None:
            continue
        if key == "name":
            cur = {"name": m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[key] = int(m.group(2))
    return rows


def loop_counts(asm):
    """{mangled name: counts} for the main MFMA loop of each kernel."""
    out = {}
    for func in re.split(r"\n(?=[A-Za-z_]\w*:\s)", asm):
        m = re.match(r"(\w+):", func)
        if not m or "v_mfma" not in func:
            continue
        ins = []
        for line in func.splitlines():
            line = line.split(";")[0].strip()
            if line and (not line.startswith(".") or line.startswith(".LBB")):
                ins.append(line)
        label_at = {l[:-1]: i for i, l in enumerate(ins) if l.endswith(":")}
        best = None
        for i, l in enumerate(ins):
            if not (l.startswith("s_cbranch") or l.startswith("s_branch")):
                continue
            tgt = label_at.get(l.split()[-1])
            if tgt is None or tgt > i:
                continue
            n = sum(x.startswith("v_mfma") for x in ins[tgt:i + 1])
            # most MFMAs first, then the tightest span that holds them
            rank = (n, tgt - i)
            if n and (best is None or rank > best[0]):
                best = (rank, tgt, i)
        if best is None:
            continue
        body = ins[best[1]:best[2] + 1]
        out[m.group(1)] = {
            "mfma": sum(x.startswith("v_mfma") for x in body),
            "branches": sum(x.startswith(("s_cbranch", "s_branch"))
                            for x in body),
            "full_lds_waits": sum(x.startswith("s_waitcnt") and
                                  "lgkmcnt(0)" in x for x in body),
            "counted_lds_waits": sum(x.startswith("s_waitcnt") and
                                     "lgkmcnt(" in x and
                                     "lgkmcnt(0)" not in x for x in body),
            "valu": sum(x.startswith("v_") and not x.startswith("v_mfma")
                        for x in body),
        }
    return out


def analyze(src, loops=False):
    with tempfile.TemporaryDirectory() as tmp:
        asm = Path(tmp) / "out.s"
        cmd = ["hipcc", "--offload-device-only", "-S", str(src), "-o",
               str(asm), "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd + device_flags(), text=True,
                           capture_output=True)
        if r.returncode:
            sys.stderr.write(r.stderr)
            raise SystemExit(f"hipcc failed on {src}")
        rows = parse_remarks(r.stderr)
        lc = loop_counts(asm.read_text()) if loops else {}
    for row, pretty in zip(rows, demangle([x["name"] for x in rows])):
        row["file"] = Path(src).name
        row["loop"] = lc.get(row["name"])
        row["name"] = pretty
    return rows


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("files", nargs="*", help="_hip/*.hip files (default: all)")
    p.add_argument("--loops", action="store_true",
                   help="also count instructions in each MFMA kernel's loop")
    args = p.parse_args(argv)
    files = [Path(f) for f in args.files] or sorted(HIP_DIR.glob("*.hip"))
    print("| file | kernel | VGPRs | scratch B/lane | occupancy | LDS B |")
    print("|---|---|---|---|---|---|")
    loops = []
    for f in files:
        for r in analyze(f, args.loops):
            print(f"| {r['file']} | `{r['name']}` | {r['vgprs']} | "
                  f"{r['scratch']} | {r['occupancy']} | {r['lds']} |")
            if r["loop"]:
                loops.append(r)
    if loops:
        print()
        print("| kernel | MFMA | branches | full LDS waits | counted LDS "
              "waits | non-MFMA vector |")
        print("|---|---|---|---|---|---|")
        for r in loops:
            c = r["loop"]
            print(f"| `{r['name']}` | {c['mfma']} | {c['branches']} | "
                  f"{c['full_lds_waits']} | {c['counted_lds_waits']} | "
                  f"{c['valu']} |")


if __name__ == "__main__":
    main()
