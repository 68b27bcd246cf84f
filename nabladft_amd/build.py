"""Builds nabladft_amd/libnablaq.so (HIP, gfx950) in-tree with plain hipcc.

    python -m nabladft_amd.build [--force]

One object per .hip file (rebuilt only when the source or a header is newer), then one link.
hipcc cross-compiles without a GPU, so this runs in the build container; the .so travels to the
GPU box with the snapshot (it is git-ignored, not gpurun-ignored).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "csrc", "_obj")
LIB = os.path.join(HERE, "libnablaq.so")
SOURCES = ["graph.hip", "gemm.hip", "gemm_bf16.hip", "edge.hip", "molpair.hip", "updfuse.hip", "node.hip", "schnet.hip", "hblock.hip", "so3.hip", "qhnet.hip", "qhgen.hip", "gemnet_graph.hip", "gemnet.hip", "escn.hip", "equiformer.hip", "geobasis.hip", "graphormer.hip", "dimenet.hip", "lbfgs.hip", "md.hip", "vib.hip", "orbitals.hip", "orbdens.hip", "orbresp.hip", "orbsmear.hip", "orbpurify.hip", "orbbond.hip", "orblowdin.hip", "orbcomm.hip", "orbsqrt.hip", "orbfrontier.hip", "orbocc.hip", "rccl.hip", "engine.hip"]
# molpair.hip: the SLP vectoriser packs neighbouring scalar f32 operations into v_pk_* beside the matrix instructions, which costs more than it saves there
# (MI355X_MICROARCH.md, "packed f32 VALU beside MFMAs"; measured 6.51 -> 6.18 ms per step, profiles/r06_gwr_mol_variants.txt)
# md.hip: no contraction of a * b + c, so that the float64 integrator rounds like the operation-by-operation restatement it is tested against (tests/md_ref.py)
# vib.hip: the same, for the realised steps and the Hessian rows (tests/vib_ref.py)
# orbitals.hip: the rank-2 update of the tridiagonalisation keeps the matrix exactly symmetric only if v_i w_j + w_i v_j is two products and one sum; the
# kernels call fma() where they want one
# orbdens.hip: the same setting as the solver it follows; its sums are written with fma() and the matrix instruction
# orbresp.hip: the same, for the density response that follows both (from here on every file takes the molecule lookup, the workgroup sum and maximum and
# the host-side launch check from orbstate.h, and the product tiles and the symmetrise tile routine from orbresp_tiles.h)
# orbsmear.hip: the same, for the smeared occupations and their response (it shares orbresp_tiles.h with orbresp.hip)
# orbpurify.hip: the same, for the purification and its response: 2 X - Y and the mirrored tiles keep X exactly symmetric (it shares orbresp_tiles.h too)
# orbbond.hip: the same, for the bond orders that follow a density: its pair sums are written with fma() and the matrix instruction (orbresp_tiles.h again)
# orblowdin.hip: the same, for the Löwdin functions of S and their reverse: K = 1 / (a_i + a_j) is a sum and a division as written (it shares the run-time-oriented
# operand tiles of orbbond_tiles.h with orbbond.hip; its symmetrise kernel is the tile routine of orbresp_tiles.h)
# orbcomm.hip: the same, for the commutators of the SCF residual: the difference of its two contractions is taken inside the accumulators as written (it
# shares orbbond_tiles.h too; its antisymmetrise kernel is the same tile routine with the other sign)
# orbsqrt.hip: the same, for the Newton-Schulz square roots: (3 I - Z Y) / 2 is a difference and a product as written, so that T is the mirrored number on both
# sides of the diagonal (it shares orbresp_tiles.h with orbpurify.hip)
# orbfrontier.hip: the same, for the projected Lanczos recurrence of the frontier levels: its sums are written with fma(), and c_i c_j is one product on both
# sides of the diagonal (it includes orbbond_tiles.h for the tiles' constants; its molecule lookup is orbstate.h's)
# orbocc.hip: the same, for the projector's Cholesky factor and the occupied levels: its column sums are written with fma() in the order of the rows, and the
# reduced matrix is the mirrored number on both sides of the diagonal (its products are rs_gemm of orbresp_tiles.h)
EXTRA = {"molpair.hip": ["-fno-slp-vectorize"], "md.hip": ["-ffp-contract=off"], "vib.hip": ["-ffp-contract=off"], "orbitals.hip": ["-ffp-contract=off"], "orbdens.hip": ["-ffp-contract=off"], "orbresp.hip": ["-ffp-contract=off"], "orbsmear.hip": ["-ffp-contract=off"], "orbpurify.hip": ["-ffp-contract=off"], "orbbond.hip": ["-ffp-contract=off"], "orblowdin.hip": ["-ffp-contract=off"], "orbcomm.hip": ["-ffp-contract=off"], "orbsqrt.hip": ["-ffp-contract=off"], "orbfrontier.hip": ["-ffp-contract=off"], "orbocc.hip": ["-ffp-contract=off"]}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=on", "-Wall", "-Wno-unused-function"]


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "lanes.h"), os.path.join(CSRC, "gemm_tile.h"), os.path.join(CSRC, "gemm_split.h"), os.path.join(CSRC, "cg_l4.inc"), os.path.join(CSRC, "devstate.h"), os.path.join(CSRC, "orbstate.h"), os.path.join(CSRC, "orbresp_tiles.h"), os.path.join(CSRC, "orbbond_tiles.h"), os.path.join(CSRC, "orbsmear_math.h"), os.path.join(os.path.dirname(HERE), "include", "nablaq.h")]
    objs, procs = [], []
    for s in SOURCES:
        src, obj = os.path.join(CSRC, s), os.path.join(OBJ, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _newer(obj, [src] + headers):
            cmd = [hipcc] + FLAGS + EXTRA.get(s, []) + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = False
    for s, p in procs:
        out, _ = p.communicate()
        if out.strip() and verbose:
            print(out)
        if p.returncode != 0:
            print(f"hipcc failed on {s}:\n{out}", file=sys.stderr)
            failed = True
    if failed:
        raise RuntimeError("hipcc compilation failed")
    if force or procs or _newer(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print("built", LIB)
