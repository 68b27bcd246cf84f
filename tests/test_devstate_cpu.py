"""CPU: the state-buffer layouts of the four device-resident jobs (``nq_lbfgs_`` / ``nq_md_`` / ``nq_vib_`` / ``nq_orb_state_layout`` and ``_state_bytes``,
built through csrc/devstate.h).  The layout functions are host-only.  Every offset and the total are compared with a restatement written here -- a table of
part byte counts and the running sum aligned up to 16 -- and with literal offsets and totals RECORDED from a build of the commit before the layouts
moved into devstate.h (10513da, the same dimensions through the same entry points): they catch a part reordered in both the code and the restatement.

Dimensions are chosen so that padding matters: B = 3 (B * 4, (B + 1) * 8 + ... end off a 16-byte boundary), N = 7 (md's byte-sized ``fixed`` part is 7 bytes,
N * 24 = 168 is 8 past a boundary), an odd D / 3, and md with every valid flag combination, rings switched off with a non-zero capacity included."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from nabladft_amd.build import build
    build(verbose=False)
    from nabladft_amd import _lib
    return _lib.load()


def running_sum(part_bytes):
    offsets, o = [], 0
    for nbytes in part_bytes:
        offsets.append(o)
        o = (o + nbytes + 15) // 16 * 16
    return offsets, o


def lbfgs_parts(N, B, memory):
    # header int32[16], mol_ptr, order, converged, rho f64[memory][B], r, r0, f0 f64[N][3], S, Y f64[memory][N][3]
    return [16 * 4, (B + 1) * 4, B * 4, B * 4, memory * B * 8, N * 24, N * 24, N * 24, memory * N * 24, memory * N * 24]


def md_parts(N, B, log_cap, frame_cap, flags):
    # a ring whose flag is off takes no room, whatever its capacity; velocity frames need flag 4 on top of the frame ring
    log_cap = log_cap if flags & 1 else 0
    frame_cap = frame_cap if flags & 2 else 0
    # header int32[32], mol_ptr, order, mol_key int64[B], mass f64[N], fixed uint8[N], r, v, rv f64[N][3], log f64[log_cap][B][8], frames, velocity frames
    return [32 * 4, (B + 1) * 4, B * 4, B * 8, N * 8, N, N * 24, N * 24, N * 24, log_cap * B * 8 * 8, frame_cap * N * 24, frame_cap * N * 24 if flags & 4 else 0]


def vib_parts(N, B, D, P):
    # header int32[16], mol_ptr, dof_ptr, hess_ptr int64[B+1], order, free_atom[D/3], disp_mol[D], disp_off int64[D+1], im f64[D], r f64[N][3], h f64[D],
    # asymmetry f64[B], sweeps, status int32[B], omega2 f64[D], work, hessian, modes f64[P]
    return [16 * 4, (B + 1) * 4, (B + 1) * 4, (B + 1) * 8, B * 4, (D // 3) * 4, D * 4, (D + 1) * 8, D * 8, N * 24, D * 8, B * 8, B * 4, B * 4, D * 8, P * 8, P * 8, P * 8]


def orb_parts(B, M, P):
    # header int32[16], orb_ptr, pack_ptr int64[B+1], order, status, info, iters int32[B], eps f64[M], coeff, work, chol f64[P]
    return [16 * 4, (B + 1) * 4, (B + 1) * 8, B * 4, B * 4, B * 4, B * 4, M * 8, P * 8, P * 8, P * 8]


# (job, dimensions, restatement, (offsets, total) recorded from the parent build)
CASES = [
    ("lbfgs", (7, 3, 2), lbfgs_parts, ([0, 64, 80, 96, 112, 160, 336, 512, 688, 1024], 1360)),
    ("lbfgs", (1, 1, 1), lbfgs_parts, ([0, 64, 80, 96, 112, 128, 160, 192, 224, 256], 288)),
    ("md", (7, 3, 2, 3, 0), md_parts, ([0, 128, 144, 160, 192, 256, 272, 448, 624, 800, 800, 800], 800)),
    ("md", (7, 3, 2, 3, 1), md_parts, ([0, 128, 144, 160, 192, 256, 272, 448, 624, 800, 1184, 1184], 1184)),
    ("md", (7, 3, 2, 3, 2), md_parts, ([0, 128, 144, 160, 192, 256, 272, 448, 624, 800, 800, 1312], 1312)),
    ("md", (7, 3, 2, 3, 3), md_parts, ([0, 128, 144, 160, 192, 256, 272, 448, 624, 800, 1184, 1696], 1696)),
    ("md", (7, 3, 2, 3, 6), md_parts, ([0, 128, 144, 160, 192, 256, 272, 448, 624, 800, 800, 1312], 1824)),
    ("md", (7, 3, 2, 3, 7), md_parts, ([0, 128, 144, 160, 192, 256, 272, 448, 624, 800, 1184, 1696], 2208)),
    ("md", (7, 3, 0, 0, 0), md_parts, ([0, 128, 144, 160, 192, 256, 272, 448, 624, 800, 800, 800], 800)),
    ("vib", (7, 3, 15, 81), vib_parts, ([0, 64, 80, 96, 128, 144, 176, 240, 368, 496, 672, 800, 832, 848, 864, 992, 1648, 2304], 2960)),
    ("vib", (7, 3, 0, 0), vib_parts, ([0, 64, 80, 96, 128, 144, 144, 144, 160, 160, 336, 336, 368, 384, 400, 400, 400, 400], 400)),
    ("orb", (3, 7, 21), orb_parts, ([0, 64, 80, 112, 128, 144, 160, 176, 240, 416, 592], 768)),
    ("orb", (1, 1, 1), orb_parts, ([0, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208], 224)),
]


@pytest.mark.parametrize("job,dims,parts,recorded", CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1]))}" for c in CASES])
def test_layout_matches_restatement_and_parent(lib, job, dims, parts, recorded):
    part_bytes = parts(*dims)
    want_offsets, want_total = running_sum(part_bytes)
    off = (C.c_size_t * len(part_bytes))()
    assert getattr(lib, f"nq_{job}_state_layout")(*dims, off) == 0, lib.nq_last_error()
    total = getattr(lib, f"nq_{job}_state_bytes")(*dims)
    assert (list(off), total) == (want_offsets, want_total)
    assert (list(off), total) == recorded


def test_part_counts_match_the_python_tables():
    """The one ``(name, dtype, shape)`` table of each state class lists as many parts as the restatement above (read from the source: the classes need a GPU)."""
    import ast
    import inspect
    from nabladft_amd import md, optimization, orbitals, vibrations
    for cls, n in ((optimization.LBFGSState, 10), (md.MDState, 12), (vibrations.VibState, 18), (orbitals.OrbitalState, 11)):
        tree = ast.parse(inspect.getsource(inspect.getmodule(cls)))
        init = next(f for c in ast.walk(tree) if isinstance(c, ast.ClassDef) and c.name == cls.__name__ for f in c.body if getattr(f, "name", "") == "__init__")
        call = next(c for c in ast.walk(init) if isinstance(c, ast.Call) and getattr(c.func, "attr", "") == "_allocate")
        assert len(call.args[2].elts) == n, cls.__name__
