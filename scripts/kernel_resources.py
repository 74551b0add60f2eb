"""A refactor's resource check: for every GPU function whose code differs between two builds of librsrl_hip.so, the code object's own
metadata side by side -- VGPRs (accumulation registers included), SGPRs, scratch bytes, spills, LDS, the waves per SIMD the register
allocation admits -- and the static instruction count.  Markdown rows on stdout; exit status 1 if a function gained scratch or spills or
lost a wave.
    python scripts/kernel_resources.py <parent.so> [<new.so>]"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from rsrl_amd import _build, _kdigest  # noqa: E402

KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count",
        ".group_segment_fixed_size")


def _tool(name):
    return os.path.join(os.path.dirname(_build._tool("clang")), name)


def resources(lib):
    """{function: dict of KEYS + 'instrs'} over every gfx950 code object of the library"""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for n, elf in enumerate(_kdigest._code_objects(open(lib, "rb").read())):
            path = os.path.join(td, f"{n}.co")
            open(path, "wb").write(elf)
            notes = subprocess.run([_tool("llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
            for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                block = ".agpr_count:" + block
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                out[name] = {k: int(re.search(re.escape(k) + r":\s+(\d+)", block).group(1)) for k in KEYS}
            dis = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n((?:.+\n)*)", dis, flags=re.M):
                if m.group(1) in out:
                    out[m.group(1)]["instrs"] = sum(1 for ln in m.group(2).split("\n") if ln.startswith("\t"))
    return out


def waves(r):
    """waves per SIMD by the unified register file: 512 registers per lane, allocated in blocks of 8, at most 8 waves"""
    return min(8, 512 // max(8, -(-r[".vgpr_count"] // 8) * 8))      # .vgpr_count is the unified total, .agpr_count its accumulation part


def main():
    parent, new = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else _build.LIB_PATH)
    moved = _kdigest.differing_functions(parent, new)
    a, b = resources(parent), resources(new)
    # (resources() splits the metadata note at each kernel's first key: if the emitter's key order ever changes it finds nothing -- say so)
    unparsed = [n for n in moved if n not in a and n not in b]
    if unparsed:
        sys.exit(f"kernel_resources: no metadata parsed for {len(unparsed)} of {len(moved)} moved functions (metadata layout changed?)")
    bad = 0
    print("| kernel | VGPR (of which AGPR) | SGPR | scratch B | spills v/s | LDS B | waves/SIMD | instrs |")
    print("|---|---|---|---|---|---|---|---|")
    for name in moved:
        p, q = a.get(name), b.get(name)
        if p is None or q is None:
            print(f"| {name} | only in {'new' if p is None else 'parent'} |")
            bad += 1
            continue
        short = re.sub(r"^_ZN4rsrl\d+", "", name)
        short = re.sub(r"EEvNS_6Common.*$", "", short)
        cell = lambda f: f"{f(p)} -> {f(q)}" if f(p) != f(q) else f"{f(p)}"  # noqa: E731
        worse = (q[".private_segment_fixed_size"] > p[".private_segment_fixed_size"] or q[".vgpr_spill_count"] > p[".vgpr_spill_count"] or
                 q[".sgpr_spill_count"] > p[".sgpr_spill_count"] or waves(q) < waves(p))
        bad += worse
        print(f"| {short}{' **!**' if worse else ''} | " + " | ".join((
            cell(lambda r: f"{r['.vgpr_count']} ({r['.agpr_count']})"), cell(lambda r: r[".sgpr_count"]),
            cell(lambda r: r[".private_segment_fixed_size"]), cell(lambda r: f"{r['.vgpr_spill_count']}/{r['.sgpr_spill_count']}"),
            cell(lambda r: r[".group_segment_fixed_size"]), cell(waves), cell(lambda r: r.get("instrs")))) + " |")
    print(f"\n{len(moved)} functions moved, {bad} break a condition")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
