#!/usr/bin/env python3
"""Instruction stream and resource line of every kernel of the .hip files given: one JSON line per kernel.

    python tools/kernel_streams.py [--diag] [--dump DIR] multimodal_embeddings_amd/csrc/attention.hip ...

For a change that must leave a kernel's machine code alone (a refactor: same bits and same speed by construction) the
lines of two trees must be EQUAL for that kernel.  Each file is compiled with the build's own FLAGS (build.py; --diag adds
-DMME_DIAG), `--save-temps` and `-Rpass-analysis=kernel-resource-usage` into a temporary directory.  A line holds the
mangled name, the instruction count, a sha256 of the normalised stream, and VGPR, AGPR, SGPR, scratch bytes per lane, LDS
bytes per block and occupancy as the compiler reports them.

The normalised stream is what stands between the kernel's label and its last s_endpgm: comments stripped, whitespace
collapsed, assembler directives dropped, `.LBB<n>_` rewritten to `.LBB_` (<n> is the function's index in its file, which
moves when a kernel is added in front of it).  Branch labels stay in the stream but are not counted as instructions.
`--dump DIR` writes one `<file>.<mangled name>.s` per kernel, so that two trees can be compared with `diff`.

The tool hashes and prints; it judges nothing.  Needs hipcc, no GPU.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the remark block of one function, in the order the compiler prints it
FIELDS = {"VGPRs": "vgpr", "AGPRs": "agpr", "TotalSGPRs": "sgpr", "ScratchSize [bytes/lane]": "scratch",
          "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}


def resources(stderr: str) -> dict:
    """mangled name -> {vgpr, agpr, sgpr, scratch, lds, occupancy} from the kernel-resource-usage remarks"""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: \S+\s+([A-Za-z][A-Za-z \[\]/]*): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = int(val)
    return out


def stream(asm: list, name: str) -> list:
    """normalised lines of kernel `name` in the device assembly `asm` (a list of lines)"""
    begin = next(i for i, raw in enumerate(asm) if raw.startswith(name + ":")) + 1
    lines = []
    for raw in asm[begin:]:
        if raw.startswith(".Lfunc_end"):
            break
        text = " ".join(raw.split(";", 1)[0].split())
        if not text or (text.startswith(".") and not text.endswith(":")):
            continue  # blank, comment or directive
        lines.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    last = max(i for i, t in enumerate(lines) if t == "s_endpgm")
    return lines[: last + 1]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="+", help=".hip files (their headers are found beside them)")
    ap.add_argument("--diag", action="store_true", help="compile with -DMME_DIAG, as build --diag does")
    ap.add_argument("--dump", metavar="DIR", help="write the normalised streams there")
    args = ap.parse_args(argv)

    from multimodal_embeddings_amd import build

    flags = build.FLAGS + (["-DMME_DIAG"] if args.diag else [])
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    for path in args.files:
        path = os.path.abspath(path)
        base = os.path.basename(path)
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([build._hipcc(), *flags, "--save-temps", "-Rpass-analysis=kernel-resource-usage", "-c", path, "-o", "out.o"],
                               cwd=tmp, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"kernel_streams: {base} does not compile\n{r.stderr}")
            (asm_file,) = [f for f in os.listdir(tmp) if f.endswith(".s") and "amdgcn" in f]
            with open(os.path.join(tmp, asm_file)) as fh:
                asm = [line.strip() for line in fh]
        kernels = {line.split()[1] for line in asm if line.startswith(".amdhsa_kernel ")}
        for name, res in resources(r.stderr).items():
            if name not in kernels:
                continue
            lines = stream(asm, name)
            text = "\n".join(lines) + "\n"
            row = {"file": base, "kernel": name, "instructions": sum(not t.endswith(":") for t in lines),
                   "sha256": hashlib.sha256(text.encode()).hexdigest(), **res}
            print(json.dumps(row), flush=True)
            if args.dump:
                with open(os.path.join(args.dump, f"{base}.{name}.s"), "w") as fh:
                    fh.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
