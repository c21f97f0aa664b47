"""Digest of every kernel's device code: the check that a move of kernels between sources changed none of them.

    python tools/kernel_digest.py [--rev REV] > listing

Compiles every csrc/*.hip of the working tree (or of git revision REV) for the device alone, with the product's flags,
and prints one sorted line per kernel: name, sha256 of the function's bytes, sha256 of its 64-byte kernel descriptor.
Bytes 16-23 of the descriptor are the entry offset (where in the object the function lies) and count as zero.  Two
listings are compared as multisets of lines: the source a kernel sits in does not enter.  CPU only; nothing is
disassembled.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from cesm_emulator_amd import build  # noqa: E402

READELF = Path(build.HIPCC).resolve().parent.parent / "llvm" / "bin" / "llvm-readelf"


def run(cmd) -> str:
    r = subprocess.run(list(map(str, cmd)), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{cmd[0]} failed:\n{r.stderr}")
    return r.stdout


def kernels(src: Path, tmp: Path) -> list:
    """(name, function digest, descriptor digest) of every kernel of one source."""
    co = tmp / (src.stem + ".co")
    cmd = build.compile_cmd(src, tmp, ["--cuda-device-only", "--no-gpu-bundle-output"])
    run(cmd[:-1] + [co])
    blob = co.read_bytes()
    sect, syms = {}, {}  # section index -> (address, file offset); symbol -> (value, size, section index)
    for line in run([READELF, "-sW", "-SW", co]).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\] \S+\s+\S+\s+([0-9a-f]{16}) ([0-9a-f]+) ", line)  # [Nr] Name Type Address Off
        if m:
            sect[int(m[1])] = (int(m[2], 16), int(m[3], 16))
        w = line.split()  # Num: Value Size Type Bind Vis Ndx Name
        if len(w) == 8 and w[3] in ("FUNC", "OBJECT") and w[6].isdigit():
            syms[w[7]] = (int(w[1], 16), int(w[2]), int(w[6]))

    def data(name):
        value, size, ndx = syms[name]
        off = sect[ndx][1] + value - sect[ndx][0]
        return bytearray(blob[off:off + size])

    out = []
    for name in syms:
        if name.endswith(".kd") and name[:-3] in syms:
            kd = data(name)
            assert len(kd) == 64, (name, len(kd))
            kd[16:24] = bytes(8)
            out.append((name[:-3], hashlib.sha256(data(name[:-3])).hexdigest(), hashlib.sha256(kd).hexdigest()))
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rev", help="digest csrc of this git revision instead of the working tree")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        srcs = build._rev_sources(a.rev, (), tmp / "src") if a.rev else build.sources()
        with cf.ThreadPoolExecutor(max_workers=8) as ex:
            rows = [k for ks in ex.map(lambda s: kernels(s, tmp), srcs) for k in ks]
        for line in sorted(" ".join(k) for k in rows):
            print(line)


if __name__ == "__main__":
    main()
