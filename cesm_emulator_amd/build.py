"""Build libcesm_hip.so (gfx950) in-tree: one hipcc compile per csrc/*.hip, linked with hipcc.

Usage: python -m cesm_emulator_amd.build [--force]
       python -m cesm_emulator_amd.build --variant NAME [--flags "..."] [--plain] [--rev REV [FILE ...]]
The second form builds an A/B library libcesm_hip_NAME.so with the same commands (build_variant).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import shlex
import shutil
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


def sources() -> list:
    return sorted(CSRC.glob("*.hip"))


def compile_cmd(src: Path, obj_dir: Path = OBJ, extra_flags=(), per_source: bool = True) -> list:
    """The hipcc command of one source: build() and build_variant() compile with nothing else.  The per-source flags go
    by the file's name, wherever the file lies."""
    special = ((["-fno-slp-vectorize"] if src.name in NO_SLP else []) +
               (["-fno-honor-nans"] if src.name in NO_NANS else [])) if per_source else []
    return [HIPCC, *FLAGS, *special, *extra_flags, "-c", str(src), "-o", str(obj_dir / (src.stem + ".o"))]


def _compile(src: Path, obj_dir: Path, extra_flags, per_source: bool) -> Path:
    out = obj_dir / (src.stem + ".o")
    # every header counts for every source (no per-source include scan): an edit to one rebuilds all
    deps = [src, *src.parent.glob("*.h"), ROOT / "include" / "cesm_hip.h", Path(__file__)]
    if out.exists() and all(out.stat().st_mtime >= d.stat().st_mtime for d in deps):
        return out
    r = subprocess.run(compile_cmd(src, obj_dir, extra_flags, per_source), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src.name}:\n{r.stderr}")
    return out


def _compile_all(srcs: list, obj_dir: Path = OBJ, extra_flags=(), per_source: bool = True) -> list:
    with cf.ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        return list(ex.map(lambda s: _compile(s, obj_dir, extra_flags, per_source), srcs))


def _link(objs: list, lib: Path) -> None:
    # link next to the library and rename over it: a reader (a running process, a tree snapshot) sees the old
    # or the new file, never a partly written one
    # (a per-process temp name: two concurrent builds must not link into the same file)
    tmp = lib.with_name(f"{lib.name}.{os.getpid()}.tmp")
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--no-undefined", *map(str, objs), "-o", str(tmp)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr}")
    os.replace(tmp, lib)


def build(force: bool = False) -> Path:
    OBJ.mkdir(parents=True, exist_ok=True)
    if force:
        for o in OBJ.glob("*.o"):
            o.unlink()
    objs = _compile_all(sources())
    if force or not LIB.exists() or any(o.stat().st_mtime > LIB.stat().st_mtime for o in objs):
        _link(objs, LIB)
    return LIB


def variant_dir(name: str) -> Path:
    return ROOT / "build" / f"var_{name}"


def variant_lib(name: str) -> Path:
    return PKG / f"libcesm_hip_{name}.so"


def _rev_sources(rev: str, files, dst: Path) -> list:
    """Fill dst with the sources and headers of csrc at git revision rev or, if files are named, with the working
    tree's and only those files from rev; returns the *.hip there."""
    rel = CSRC.relative_to(ROOT).as_posix()

    def git(*args):
        r = subprocess.run(["git", "-C", str(ROOT), *args], capture_output=True)
        if r.returncode != 0:
            raise RuntimeError(f"git {' '.join(args)}: {r.stderr.decode().strip()}")
        return r.stdout

    dst.mkdir(parents=True)
    if files:
        for f in [*sources(), *CSRC.glob("*.h")]:
            shutil.copy2(f, dst)
    else:
        listed = git("ls-tree", "--name-only", rev, rel + "/").decode().split("\n")
        files = [Path(n).name for n in listed if n.endswith((".hip", ".h"))]
    for f in files:
        (dst / f).write_bytes(git("show", f"{rev}:{rel}/{f}"))  # a file that rev lacks is an error
    return sorted(dst.glob("*.hip"))


def build_variant(name: str, extra_flags=(), per_source: bool = True, rev=None, files=()) -> Path:
    """A/B library cesm_emulator_amd/libcesm_hip_<name>.so (load it with CESM_HIP_LIB=<path>): the product's compile
    commands plus extra_flags, without the per-source flags if per_source is false; objects under build/var_<name>,
    always compiled afresh.

    rev alone: the csrc/*.hip and csrc/*.h of that git revision, whatever its set of files.  rev and files: the
    working tree's sources with the named files taken from rev.  Flags and include/cesm_hip.h are the working tree's."""
    if files and rev is None:
        raise ValueError("files need a rev")
    var = variant_dir(name)
    shutil.rmtree(var, ignore_errors=True)
    var.mkdir(parents=True)
    srcs = _rev_sources(rev, files, var / "src") if rev is not None else sources()
    _link(_compile_all(srcs, var, extra_flags, per_source), variant_lib(name))
    return variant_lib(name)


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
    ap = argparse.ArgumentParser(prog="python -m cesm_emulator_amd.build")
    ap.add_argument("--force", action="store_true", help="recompile every source of libcesm_hip.so")
    ap.add_argument("--variant", metavar="NAME", help="build libcesm_hip_NAME.so instead (build_variant)")
    ap.add_argument("--flags", default="", help='extra compile flags of the variant, one word: --flags "-DA -DB"')
    ap.add_argument("--plain", action="store_true", help="variant without the per-source flags")
    ap.add_argument("--rev", nargs="+", metavar=("REV", "FILE"), help="variant sources from git revision REV: all "
                    "of csrc, or the working tree's with only the named FILEs from REV (every word after REV is a FILE: "
                    "give --rev last)")
    argv = sys.argv[1:]
    for i, w in enumerate(argv[:-1]):
        if w == "--flags":  # argparse takes a separate value that begins with "-" for an option: join the two
            argv[i:i + 2] = [f"--flags={argv[i + 1]}"]
            break
    a = ap.parse_args(argv)
    if a.variant is None:
        if a.flags or a.plain or a.rev:
            ap.error("--flags, --plain and --rev need --variant")
        print(build(force=a.force))
    else:
        rev, *files = a.rev or [None]
        print(build_variant(a.variant, shlex.split(a.flags), not a.plain, rev, files))
