"""CPU: the surface of the ``optimize`` job (nabladft_amd/optimization.py, ABI 17) and the float64 numpy restatement of one optimiser step
(tests/lbfgs_helpers.py) against what the real reference did (tests/golden/lbfgs_*.npz, scripts/make_golden_lbfgs.py).  The restatement is the yardstick of
the random operator cases in tests/test_optimization_gpu.py, so it is pinned to the reference here: teacher-forced, step by step, within 10 x the fixture's
``reorder_spread`` (what the reference itself moves by when only its summation order changes)."""
import ctypes as C
import os
import shutil
import sqlite3

import numpy as np
import pytest
import torch

from lbfgs_helpers import LbfgsNumpy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    fx = dict(np.load(os.path.join(GOLDEN, f"lbfgs_{name}.npz")))
    fx["f"] = np.load(os.path.join(GOLDEN, f"lbfgs_{name}_forces.npz"))["f"]
    return fx


@pytest.fixture(scope="module")
def lib():
    from nabladft_amd.build import build
    build(verbose=False)
    from nabladft_amd import _lib
    return _lib.load()


def test_symbols_bound_and_abi_version(lib):
    from nabladft_amd import _lib
    for name in ("nq_lbfgs_state_bytes", "nq_lbfgs_state_layout", "nq_lbfgs_init", "nq_lbfgs_step"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 17 == lib.nq_abi_version()
    import nabladft_amd as nq
    assert nq.ASEBatchwiseLBFGS is nq.optimization.ASEBatchwiseLBFGS and nq.PyGBatchwiseCalculator and nq.BatchwiseOptimizeTask


def test_state_size_and_layout(lib):
    N, B, m = 351, 7, 100
    total = lib.nq_lbfgs_state_bytes(N, B, m)
    off = (C.c_size_t * 10)()
    assert lib.nq_lbfgs_state_layout(N, B, m, off) == 0
    off = list(off)
    assert off == sorted(off) and all(o % 16 == 0 for o in off)
    assert total >= off[9] + m * N * 24 and total - off[9] - m * N * 24 < 16
    assert off[9] - off[8] >= m * N * 24 and off[5] - off[4] >= m * B * 8            # the rings: [memory][N][3] and [memory][B] float64
    # the issue's bench batch: 2 x 205 MB of history
    assert 2 * 205e6 < lib.nq_lbfgs_state_bytes(85600, 2048, 100) < 2 * 205e6 * 1.05


def test_argument_errors_are_host_side(lib):
    """Molecules above 512 atoms, memory < 1, maxstep <= 0: error code + text.  Every call here returns from the host-side argument checks, before any HIP
    call, so host buffers can stand in for device arrays (tests/test_optimization_gpu.py repeats the cases with device buffers and checks nothing was written)."""
    assert lib.nq_lbfgs_state_bytes(10, 1, 0) == 0 and b"memory=0" in lib.nq_last_error()
    host = (C.c_double * 4096)()
    dummy = C.addressof(host) // 16 * 16 + 16
    n_small = C.c_int32(-1)
    ptr = np.array([0, 513], dtype=np.int32)
    args = lambda p, n, mem: (dummy, 1 << 30, p.ctypes.data_as(C.c_void_p), n, len(p) - 1, mem, dummy, 0, dummy, C.byref(n_small), None)
    assert lib.nq_lbfgs_init(*args(ptr, 513, 10)) == 3                      # NQ_ERR_MOL_TOO_LARGE
    assert b"513 atoms" in lib.nq_last_error()
    ptr = np.array([0, 5, 12], dtype=np.int32)
    assert lib.nq_lbfgs_init(*args(ptr, 12, 0)) == 2 and b"memory=0" in lib.nq_last_error()
    assert lib.nq_lbfgs_init(*args(ptr, 13, 4)) == 2 and b"mol_ptr" in lib.nq_last_error()
    step = lambda maxstep, mem=4: lib.nq_lbfgs_step(dummy, 12, 2, mem, 2, dummy, 0, None, dummy, 0.05, maxstep, 1.0, 1.0, 0, None)
    assert step(0.0) == 2 and b"maxstep" in lib.nq_last_error()
    assert step(-0.2) == 2
    assert step(0.2, mem=0) == 2 and b"memory=0" in lib.nq_last_error()
    assert n_small.value == -1


def test_config_dicts_instantiate_the_mirrors():
    """config/optimizer/batchwise_lbfgs.yaml and config/calculator/pyg_calculator.yaml with only the _target_ lines changed."""
    import importlib
    optimizer_yaml = {"_target_": "nabladft_amd.optimization.ASEBatchwiseLBFGS", "master": True, "use_line_search": False}
    calculator_yaml = {"_target_": "nabladft_amd.optimization.PyGBatchwiseCalculator", "device": "cpu", "energy_unit": "Hartree", "position_unit": "Ang"}

    def instantiate(cfg, **extra):
        mod, cls = cfg["_target_"].rsplit(".", 1)
        return getattr(importlib.import_module(mod), cls)(**{k: v for k, v in cfg.items() if k != "_target_"}, **extra)

    calc = instantiate(calculator_yaml, model=lambda b: (torch.zeros(1), torch.zeros_like(b.pos)))
    opt = instantiate(optimizer_yaml, calculator=calc)
    assert (opt.memory, opt.maxstep, opt.damping, opt.H0, opt.check_every) == (100, 0.2, 1.0, 1.0, 1)        # the reference's defaults
    assert calc.property_units == {"energy": 1.0, "forces": 1.0} and calc.results is None


def test_unbuilt_options_raise(lib):
    from nabladft_amd.optimization import ASEBatchwiseLBFGS, PyGBatchwiseCalculator
    model = lambda b: None
    calc = PyGBatchwiseCalculator(model, "cpu", energy_unit="Hartree", position_unit="Angstrom")
    with pytest.raises(NotImplementedError):
        ASEBatchwiseLBFGS(calc, use_line_search=True)
    with pytest.raises(NotImplementedError):
        ASEBatchwiseLBFGS(calc, restart="lbfgs.pckl")
    with pytest.raises(NotImplementedError):
        ASEBatchwiseLBFGS(calc, trajectory="traj")
    with pytest.raises(ValueError, match="much too large"):
        ASEBatchwiseLBFGS(calc, maxstep=1.5)
    with pytest.raises(NotImplementedError):
        PyGBatchwiseCalculator(model, "cpu", energy_unit="eV", position_unit="Ang")
    with pytest.raises(NotImplementedError):
        PyGBatchwiseCalculator(model, "cpu")                                             # the reference's default unit is eV
    with pytest.raises(NotImplementedError):
        PyGBatchwiseCalculator(model, "cpu", energy_unit="Hartree", position_unit="Bohr")
    opt = ASEBatchwiseLBFGS(calc, logfile=None)
    from nabladft_amd import Batch
    with pytest.raises(RuntimeError, match="MI355X only"):                                # no CPU fallback
        opt.run(Batch(torch.zeros(3, 3), torch.ones(3, dtype=torch.long), torch.zeros(3, dtype=torch.long)))


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_numpy_restatement_reproduces_the_reference(case):
    fx = load_case(case)
    tol = 10 * float(fx["reorder_spread"])
    fixed = fx["fixed"] if fx["fixed"].size else None
    opt = LbfgsNumpy(fx["ptr"], memory=int(fx["memory"]), maxstep=float(fx["maxstep"]), fixed=fixed)
    K = int(fx["nsteps"])
    assert fx["r"].shape[0] == K + 1 and fx["mask"].shape[0] == K
    worst = 0.0
    for k in range(K):
        new = opt.step(fx["r"][k], fx["f"][k], float(fx["fmax"]))
        assert np.array_equal(opt.mask, fx["mask"][k]), k
        assert opt.n_normalizations == int(fx["nnorm"][k]), k
        worst = max(worst, float(np.abs(new - fx["r"][k + 1]).max()))
    print(f"case {case}: {K} steps, worst |dr| {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol
    rho = np.array(opt.rho)
    assert rho.shape == fx["rho"].shape == (min(K - 1, int(fx["memory"])), len(fx["ptr"]) - 1)
    assert (np.abs(rho - fx["rho"]) <= tol * np.maximum(1.0, np.abs(fx["rho"]))).all()
    assert bool(opt.converged_mask(fx["f"][K], float(fx["fmax"])).all()) == bool(fx["converged"])
    if case == "B":
        assert K > int(fx["memory"]) and int(fx["nnorm"][-1]) > 10                      # the ring wrapped and steps were clamped
    if case == "A":
        first = [int(np.argmax(fx["mask"][:, b])) if fx["mask"][:, b].any() else K for b in range(fx["mask"].shape[1])]
        assert len(set(first)) > 3                                                        # molecules converge at different steps: the mask is exercised


# ---- the task's writer, with the restatement as the optimiser and a host callable as the model ---------------------------------------------------
class HostOptimizer:
    """BatchwiseDynamics.irun around LbfgsNumpy: what BatchwiseOptimizeTask needs of an optimiser (run, positions, calculator)."""

    def __init__(self, calculator):
        self.calculator, self.history = calculator, []

    def run(self, batch, fmax, steps):
        from nabladft_amd import Batch
        ptr = batch.ptr.numpy()
        r = batch.pos.double().numpy()
        opt = LbfgsNumpy(ptr)
        call = lambda: self.calculator.calculate(Batch(torch.from_numpy(r).float(), batch.z, batch.batch, ptr=batch.ptr))
        call()
        n = 0
        while not opt.converged_mask(self.calculator.forces.numpy(), fmax).all() and n < steps:
            r = opt.step(r, self.calculator.forces.numpy(), fmax)
            n += 1
            call()
        self.nsteps, self.positions = n, torch.from_numpy(r)
        self.history.append(r)
        return n < steps


def spring_model(batch):
    """E = k/2 sum |r - centroid|^2 per molecule, F = -k (r - centroid), k = 0.5."""
    B = int(batch.ptr.shape[0]) - 1
    cnt = torch.bincount(batch.batch, minlength=B).to(batch.pos.dtype)
    cen = torch.zeros(B, 3, dtype=batch.pos.dtype).index_add_(0, batch.batch, batch.pos) / cnt[:, None]
    d = batch.pos - cen[batch.batch]
    return torch.zeros(B, dtype=batch.pos.dtype).index_add_(0, batch.batch, 0.25 * d.pow(2).sum(1)), -0.5 * d


def test_task_writes_a_database_our_reader_opens(tmp_path):
    from nabladft_amd import read_energy_database
    from nabladft_amd.data import _decode_ase_blob
    from nabladft_amd.optimization import BatchwiseOptimizeTask, PyGBatchwiseCalculator, _encode_ase_blob
    src = os.path.join(GOLDEN, "energy_db_30.db")
    inp, out = str(tmp_path / "in.db"), str(tmp_path / "out.db")
    shutil.copy(src, inp)
    opt = HostOptimizer(PyGBatchwiseCalculator(spring_model, "cpu", energy_unit="Hartree", position_unit="Ang"))
    BatchwiseOptimizeTask(inp, out, opt, batch_size=8, fmax=1e-3, steps=50).run()
    assert len(opt.history) == 4 and opt.nsteps < 50                                      # 30 rows in batches of 8
    a, b = sqlite3.connect(inp), sqlite3.connect(out)
    schema = lambda c: c.execute("select type, name, sql from sqlite_master where name not like 'sqlite_%' order by name").fetchall()
    assert schema(a) == schema(b)
    cols = [r[1] for r in a.execute("pragma table_info(systems)")]
    ra, rb = [c.execute("select * from systems order by id").fetchall() for c in (a, b)]
    assert len(ra) == len(rb) == 30
    final = np.concatenate(opt.history)
    at = 0
    for x, y in zip(ra, rb):
        n = x[cols.index("natoms")]
        for name, u, v in zip(cols, x, y):
            if name not in ("positions", "data"):
                assert u == v and type(u) is type(v), name                             # byte-equal copies
        pos = np.frombuffer(y[cols.index("positions")], dtype=np.float64).reshape(-1, 3)
        assert np.array_equal(pos, final[at:at + n])
        d_in, d_out = _decode_ase_blob(x[cols.index("data")]), _decode_ase_blob(y[cols.index("data")])
        assert set(d_out) == set(d_in) | {"model_energy", "model_forces"}
        assert d_out["energy"] == d_in["energy"] and np.array_equal(d_out["forces"], d_in["forces"])
        assert isinstance(d_out["model_energy"], list) and len(d_out["model_energy"]) == 1 and isinstance(d_out["model_energy"][0], float)
        assert d_out["model_forces"].shape == (n, 3)
        cen = pos.astype(np.float32).mean(0)
        assert np.abs(d_out["model_forces"] + 0.5 * (pos.astype(np.float32) - cen)).max() < 1e-5     # this row's own atoms, not the batch's first molecule
        assert np.sqrt((d_out["model_forces"].astype(np.float64) ** 2).sum(1).max()) < 1e-3
        at += n
    a.close(), b.close()
    arena = read_energy_database(out)
    ref = read_energy_database(inp)
    assert len(arena) == 30 and torch.equal(arena.z, ref.z) and torch.equal(arena.y, ref.y) and torch.equal(arena.forces, ref.forces)
    assert torch.equal(arena.pos, torch.from_numpy(final.astype(np.float32)))
    # the encoder is the inverse of the reader on nested content too
    obj = {"a": [1.5], "b": np.arange(6, dtype=np.float64).reshape(2, 3), "c": {"d": np.array([1, 2], dtype=np.int32), "e": "text"}}
    back = _decode_ase_blob(_encode_ase_blob(obj))
    assert back["a"] == [1.5] and back["c"]["e"] == "text" and np.array_equal(back["b"], obj["b"]) and np.array_equal(back["c"]["d"], obj["c"]["d"])
    with pytest.raises(FileExistsError):
        BatchwiseOptimizeTask(inp, out, opt, batch_size=8, fmax=1e-3, steps=50).run()
