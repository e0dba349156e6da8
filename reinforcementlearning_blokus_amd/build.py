"""Build the in-tree HIP library (gfx950) and the CPU oracle (test infrastructure)."""
from __future__ import annotations

import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
SRC = os.path.join(_HERE, "csrc", "blokus_kernels.hip")
OUT = os.path.join(_HERE, "_lib", "libblokus_hip.so")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


DEPS = [SRC, os.path.join(_HERE, "csrc", "orient_table.h"), os.path.join(_HERE, "csrc", "exp_cr.h"),
        os.path.join(ROOT, "include", "blokus_hip.h")]
HASH_FILE = OUT + ".srchash"  # sha256 of the sources the .so was built from


def source_hash() -> str:
    import hashlib
    h = hashlib.sha256()
    for d in DEPS:
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def built_hash():
    try:
        with open(HASH_FILE) as f:
            return f.read().strip()
    except OSError:
        return None


# translation units of csrc/blokus_kernels.hip (its BK_U_* numbers): the C-ABI host code,
# then one unit per kernel family, compiled in parallel and linked into one .so
UNITS = {"host": 1, "movegen": 2, "rollout": 3, "rollout_fr": 4, "rollout_frh": 5, "fastmcts": 6,
         "mcts": 7, "mcts_pair": 8, "mcts_h": 9, "coop": 10, "coop_h": 11, "telemetry": 12,
         "snapshot": 13, "steplog": 14, "rollout_frhs": 15, "coop_l": 16, "gbt": 17, "coop_g": 18,
         "rollout_frhw": 19}


# per-unit code-generation flags (measured per kernel).  Machine LICM hoists
# loop-invariant address and constant computations out of the persistent loops into
# registers held for the whole kernel; without it k_rollout_fr spills 35 instead of 62
# VGPRs (+2 % frontier-order playouts/s) and k_mcts_coop_h needs 294 instead of 355
# registers (profiles/r05/sweeps/r05b, r05a)
_NO_MLICM = ("-mllvm", "-disable-machine-licm")
# Zero-column flags of the stencil classes (csrc/blokus_kernels.hip BK_CLASS_LIST): the
# lane-pair scan of k_mcts_pair pays per class, so it takes the unsplit classes with
# their shared flags; k_rollout_fr_h has no measurement and keeps the unflagged code
# (profiles/r11)
# The playout kernels and k_mcts count the stencil in phases and rebuild the second
# plane between them (BK_STENCIL_MUX), each on an A/B of its own; k_mcts_h measured no
# different with it and the dense-mask kernels of config 2 do not go through the code it
# changes, so those units keep their lists (profiles/r13)
_MUX = ("-DBK_STENCIL_MUX",)
UNIT_FLAGS = {"rollout_fr": _NO_MLICM + _MUX, "rollout": _MUX, "mcts": _MUX, "coop": _NO_MLICM, "coop_h": _NO_MLICM,
              "coop_l": _NO_MLICM,  # k_mcts_coop_l is k_mcts_coop's tree part: the same reasons
              "coop_g": _NO_MLICM,  # k_mcts_coop_g is k_mcts_coop_l with another value(): coop_l's flags
              "mcts_pair": ("-DBK_STENCIL_COMMON",), "rollout_frh": ("-DBK_STENCIL_PLAIN",),
              "rollout_frhs": ("-DBK_STENCIL_PLAIN",),  # k_rollout_fr_h's code plus the capture
              "rollout_frhw": ("-DBK_STENCIL_PLAIN",)}  # k_rollout_fr_h's code with per-set score tables


def compile_library(out: str, defines=(), verbose: bool = True, jobs: int = 0, unit_flags=None) -> str:
    """Compile every unit of csrc/blokus_kernels.hip with hipcc (gfx950) in parallel and
    link them into `out` (one fat binary per kernel unit; kernels are launched from the
    host unit through their host stubs).  unit_flags: extra hipcc flags per unit name
    (default UNIT_FLAGS)."""
    unit_flags = UNIT_FLAGS if unit_flags is None else unit_flags
    from concurrent.futures import ThreadPoolExecutor
    objdir = out + ".objs"
    os.makedirs(objdir, exist_ok=True)
    base = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-pthread",
            "-Wno-unused-command-line-argument"] + [f"-D{d}" for d in defines]

    def unit(item):
        name, u = item
        obj = os.path.join(objdir, name + ".o")
        cmd = base + list(unit_flags.get(name, ())) + [f"-DBK_TU={u}"]
        cmd += ["-c", "-o", obj, SRC]
        if verbose:
            print("[build] " + " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return obj

    jobs = jobs or min(len(UNITS), int(os.environ.get("MAX_JOBS", "0")) or (os.cpu_count() or 4))
    with ThreadPoolExecutor(max(1, jobs)) as ex:
        objs = list(ex.map(unit, sorted(UNITS.items(), key=lambda kv: kv[1])))
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-pthread", "-o", out + ".tmp"] + objs
    if verbose:
        print("[build] " + " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(out + ".tmp", out)
    shutil.rmtree(objdir, ignore_errors=True)
    return out


def build_native(force: bool = True, verbose: bool = True) -> str:
    """Compile libblokus_hip.so for gfx950 with hipcc.  Always compiles by default (the
    driver's build() check must exercise hipcc); force=False reuses an in-tree .so only
    when it was built from exactly these sources (sha256 recorded next to it)."""
    if not force and os.path.exists(OUT) and built_hash() == source_hash():
        if verbose:
            print(f"[build] reusing {OUT} (built from sources {built_hash()[:12]})", flush=True)
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    digest = source_hash()
    compile_library(OUT, verbose=verbose)
    with open(HASH_FILE, "w") as f:
        f.write(digest + "\n")
    return OUT


def build_oracle() -> None:
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


if __name__ == "__main__":
    print(build_native())
    build_oracle()
