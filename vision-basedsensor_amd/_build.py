"""Build csrc/*.hip into csrc/libvbs.so for gfx950 with hipcc (in-tree, so the .so travels with gpurun)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libvbs.so")
SOURCES = ("api.hip", "api_analysis.hip", "k_gray.hip", "k_blur_mfma.hip", "k_blur16.hip", "k_ncc_mfma.hip", "k_ncc_map.hip", "k_ncc_general.hip", "k_morph.hip", "k_label.hip", "k_finalize.hip", "labelling.hip", "k_ccl.hip", "k_stage.hip", "k_stage_lat.hip", "k_solve.hip", "k_undistort.hip", "k_ids.hip", "host_csv.hip", "host_mjpeg.hip", "k_annotate.hip", "k_jpeg_enc.hip", "k_series.hip", "k_filter.hip", "k_steps.hip", "k_pose.hip", "k_field.hip", "k_spectrum.hip", "k_envelope.hip", "k_kinematics.hip", "k_modes.hip", "k_motion.hip", "k_robust.hip", "k_jpeg_huff.hip", "k_diameter.hip", "k_pnp.hip", "k_chess.hip", "k_calib.hip", "k_retrack.hip", "k_uncert.hip", "k_posecov.hip", "k_refine.hip", "k_shape.hip", "k_rigid.hip", "k_sphere.hip", "k_rigid_ml.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]
# k_ncc_mfma.hip: no SLP pairings (they cost registers, 127 -> 108, and instructions) and no packed float32 instructions at all:
# next to matrix-core instructions a v_pk_fma_f32 costs more than the two v_fma_f32 it replaces (k_ncc_mfma 1.94 ->
# 1.90 us per frame with its float2 arithmetic split by the compiler)
# k_ncc_map.hip: the same flags only because k_ncc was built with them while it shared a file with k_ncc_mfma, and its code
# differs without them (k_nccg / k_nccg_stats in k_ncc_general.hip do not: profiles/frontend_split_text_equal.txt)
_NCC_FLAGS = ["-fno-slp-vectorize", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FILE_FLAGS = {"k_ncc_mfma.hip": _NCC_FLAGS, "k_ncc_map.hip": _NCC_FLAGS}


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, extra_flags=(), suffix: str = "") -> str:
    """`extra_flags` / `suffix`: a second library next to the product one, e.g. tools/ build `libvbs_dbg.so` with
    -DVBS_DEBUG_KNOBS (phase-timing early exits read from the environment); the product library never has them."""
    hdrs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(CSRC, "..", "..", "include", "vbs.h")]
    lib = LIB.replace(".so", suffix + ".so")
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", suffix + ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([HIPCC] + FLAGS + FILE_FLAGS.get(src, []) + list(extra_flags) + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return r.stderr

    with ThreadPoolExecutor(max_workers=4) as ex:
        for warn in ex.map(run, jobs):
            if verbose and warn:
                print(warn, file=sys.stderr)
    _check_isa(force or any("k_blur16.hip" in " ".join(j) for j in jobs), list(extra_flags), suffix, run)
    if force or jobs or _stale(lib, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", lib] + objs)
    return lib


def _check_isa(rebuilt: bool, extra_flags, suffix, run):
    """k_blur16's loader keeps loads in flight across inline-asm statements: what the register allocator did with their
    destination registers is checked in the disassembly after every (re)build of k_blur16.hip (vbs_amd/_isa_check.py says
    what is checked and why); a violation fails the build."""
    from . import _isa_check
    src = os.path.join(CSRC, "k_blur16.hip")
    asm = os.path.join(CSRC, "k_blur16" + suffix + ".s")
    stamp = asm + ".ok"
    if not rebuilt and os.path.exists(stamp) and os.path.getmtime(stamp) >= os.path.getmtime(src):
        return
    run([HIPCC] + FLAGS + FILE_FLAGS.get("k_blur16.hip", []) + extra_flags + ["--cuda-device-only", "-S", src, "-o", asm])
    problems = _isa_check.check_blur16(open(asm).read())
    os.remove(asm)
    if problems:
        if os.path.exists(stamp):
            os.remove(stamp)
        raise RuntimeError("k_blur16 ISA check failed (vbs_amd/_isa_check.py):\n  " + "\n  ".join(problems))
    open(stamp, "w").write("ok\n")


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
