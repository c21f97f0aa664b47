"""Build libcesm_hip.so (gfx950) in-tree: one hipcc compile per csrc/*.hip, linked with hipcc.

Usage: python -m cesm_emulator_amd.build [--force]
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import subprocess
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
ROOT = PKG.parent
OBJ = ROOT / "build" / "obj"
LIB = PKG / "libcesm_hip.so"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I", str(ROOT / "include")]
# Sources whose kernels apply RoPE: with the SLP vectorizer on, their results changed between identical calls (rounds
# 2-3: ~1/3 of the level-0 dx rows).  Round 5 found why (tools/vgpr_pollute_check.py, profiles/r5_pollute_slp.txt):
# the SLP-vectorized twh_bwd reads registers it has not written -- its outputs change with the contents a previous
# kernel left in the register file -- while the scalar build's do not, for any register / LDS pattern
# (tests/test_gpu_stale_state.py, tests/test_gpu_determinism.py).  So these sources stay scalar; the other sources keep
# the packed forms (their epilogues measured faster with them: conv -7 %, fused SLA forward -18 %) and pass the same
# stale-state tests.
NO_SLP = {"tblock.hip", "tflash.hip", "attn.hip"}
# Attention sources: no NaN semantics, so fmaxf after a lane permute (the softmax row maxima) needs no canonicalising
# v_max per operand (round 4, same-call A/B: SLA backward 4.92 -> 4.68 ms, forward 2.59 -> 2.51 ms at level 0).  Not
# misc.hip: its gradient-norm check relies on isfinite.
NO_NANS = {"tblock.hip", "tflash.hip", "attn.hip", "sla_fused.hip"}


def _flags(src: Path):
    return (FLAGS + (["-fno-slp-vectorize"] if src.name in NO_SLP else []) +
            (["-fno-honor-nans"] if src.name in NO_NANS else []))


def _compile(src: Path) -> Path:
    out = OBJ / (src.stem + ".o")
    # every header counts for every source (no per-source include scan): an edit to one rebuilds all
    deps = [src, *CSRC.glob("*.h"), ROOT / "include" / "cesm_hip.h", Path(__file__)]
    if out.exists() and all(out.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return out
    cmd = [HIPCC, *_flags(src), "-c", str(src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src.name}:\n{r.stderr}")
    return out


def build(force: bool = False) -> Path:
    OBJ.mkdir(parents=True, exist_ok=True)
    srcs = sorted(CSRC.glob("*.hip"))
    if force:
        for o in OBJ.glob("*.o"):
            o.unlink()
    with cf.ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        objs = list(ex.map(_compile, srcs))
    if force or not LIB.exists() or any(o.stat().st_mtime > LIB.stat().st_mtime for o in objs):
        # link next to the library and rename over it: a reader (a running process, a tree snapshot) sees the old
        # or the new file, never a partly written one
        # (a per-process temp name: two concurrent builds must not link into the same file)
        tmp = LIB.with_name(f"{LIB.name}.{os.getpid()}.tmp")
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--no-undefined", *map(str, objs), "-o", str(tmp)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
        os.replace(tmp, LIB)
    return LIB


def build_diag() -> list:
    """Test-only diagnostic libraries (tools/diag/*.hip -> tools/diag/lib<name>.so): the register / LDS polluters
    tests/test_gpu_determinism.py runs before the fused kernels.  Not part of libcesm_hip.so."""
    out = []
    for src in sorted((ROOT / "tools" / "diag").glob("*.hip")):
        so = src.with_name(f"lib{src.stem}.so")
        if not so.exists() or so.stat().st_mtime < src.stat().st_mtime:
            tmp = so.with_name(f"{so.name}.{os.getpid()}.tmp")
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", str(src), "-o", str(tmp)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed for {src.name}:\n{r.stderr}")
            os.replace(tmp, so)
        out.append(so)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
