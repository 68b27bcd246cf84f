"""nabladft_amd -- MI355X-native (gfx950, hand-written HIP) engine for the nablaDFT PaiNN hot path.

Public surface mirrors the reference plugin classes for this path:
  nabladft_amd.PaiNN            <-> nablaDFT.painn_pyg.PaiNN            (painn.py:22-148)
  nabladft_amd.PaiNNLightning   <-> nablaDFT.painn_pyg.PaiNNLightning   (painn.py:623-776)
  nabladft_amd.L2Loss           <-> nablaDFT.gemnet_oc.loss.L2Loss      (gemnet_oc/loss.py:15-22)
  nabladft_amd.QHNet            <-> nablaDFT.qhnet.QHNet                (qhnet/qhnet.py:24-342)
  nabladft_amd.QHNetLightning   <-> nablaDFT.qhnet.QHNetLightning       (qhnet/qhnet.py:345-536)
  nabladft_amd.GemNetOC         <-> nablaDFT.gemnet_oc.GemNetOC         (gemnet_oc/gemnet_oc.py:36-1340)
  nabladft_amd.GemNetOCLightning <-> nablaDFT.gemnet_oc.GemNetOCLightning (gemnet_oc/gemnet_oc.py:1343-1493)
  nabladft_amd.eSCN             <-> nablaDFT.escn.eSCN                  (escn/escn.py:36-490)
  nabladft_amd.eSCNLightning    <-> nablaDFT.escn.eSCNLightning         (escn/escn.py:1006-1159)
  nabladft_amd.EquiformerV2_OC20 <-> nablaDFT.equiformer_v2.EquiformerV2_OC20 (equiformer_v2/equiformer_v2_oc20.py:51-640)
  nabladft_amd.EquiformerV2_OC20_Lightning <-> nablaDFT.equiformer_v2.EquiformerV2_OC20_Lightning (equiformer_v2/equiformer_v2_oc20.py:643-817)
  nabladft_amd.Graphormer3D / Graphormer3DLightning <-> nablaDFT.graphormer.Graphormer3D / Graphormer3DLightning (graphormer/graphormer_3d.py:227-483)
  nabladft_amd.DimeNetPlusPlusPotential / DimeNetPlusPlusLightning <-> nablaDFT.dimenetplusplus.* (dimenetplusplus/dimenetplusplus.py:22-270; the
                                    torch-geometric core restated, unpinned)
  nabladft_amd.AtomisticTaskFixed <-> nablaDFT.ase_model.AtomisticTaskFixed (ase_model/task.py:9-73)
  nabladft_amd.ASEBatchwiseLBFGS / PyGBatchwiseCalculator / BatchwiseOptimizeTask <-> nablaDFT.optimization.* (optimizers.py:293-605, calculator.py:98-132,
                                    task.py:9-73): the `optimize` job, L-BFGS state on the device (optimization.py)
  nabladft_amd.PYGAseInterface / BatchedMD <-> nablaDFT.optimization.PYGAseInterface (pyg_ase_interface.py:119-335): single point, batched NVE / Langevin
                                    MD with the state on the device (md.py; the ase integrators restated, unpinned), relaxation through the device L-BFGS
  nabladft_amd.BatchedVibrations <-> ase.vibrations.Vibrations behind PYGAseInterface.compute_normal_modes (pyg_ase_interface.py:317-334): batched
                                    finite-difference Hessians and a Jacobi eigensolver on the device (vibrations.py; restated, unpinned)
  nabladft_amd.BatchedOrbitals / OrbitalErrors <-> the orbital_energies / orbital_coefficients slots phisnet/nn/neural_network.py:969-993 returns as zeros:
                                    batched generalized symmetric eigensolver on the device (orbitals.py; no reference code, tested against numpy)
  nabladft_amd.BatchedPurification / purified_density_matrix <-> the same slots, for the density alone: SP2 purification and its gradient from float64 matrix
                                    products, no solve (orbitals.py, orbital_loss.py; no reference code, tested against numpy and the solver route)
  nabladft_amd.bond_orders / BondOrderLoss / QHNetBondOrderLightning <-> the same slots: Mayer bond orders and atomic valences of a density matrix and their
                                    gradients (orbitals.py, orbital_loss.py; no reference code, tested against numpy and torch autograd)
  nabladft_amd.lowdin_basis / lowdin_populations / lowdin_bond_orders / lowdin_hamiltonian / QHNetLowdinLightning <-> the same slots: S^(1/2), S^(-1/2), Löwdin
                                    populations, Wiberg indices and the orthogonalised Hamiltonian with gradients that divide no difference of levels of S
                                    (orbitals.py, orbital_loss.py; no reference code, tested against numpy, scipy and torch autograd)
  nabladft_amd.scf_residual / commutator / ScfResidualLoss / scf_target / QHNetCommutatorLightning / ScfResidualErrors <-> the same slots: the SCF residual
                                    [H^L, D^L] of a predicted Hamiltonian against the target's density, a loss on the occupied subspace that solves nothing
                                    for the prediction (orbitals.py, orbital_loss.py; no reference code, tested against numpy and torch autograd)
  nabladft_amd.BatchedMatrixRoot / LowdinBasis.of(method="newton_schulz") / scf_target_iterative / scf_target_blocks <-> the same slots: S^(1/2) and
                                    S^(-1/2) by the coupled Newton-Schulz iteration and, with the SP2 purification, an SCF target without any solve
                                    (orbitals.py, orbital_loss.py; no reference code, tested against numpy, scipy and the decomposition route)
  nabladft_amd.purified_frontier / FrontierLoss / FrontierLevels / QHNetPurifiedFrontierLightning <-> the same slots, for HOMO, LUMO and the gap alone: a
                                    projected Lanczos recurrence on what the SP2 purification leaves, and the levels' gradients, no solve (orbitals.py,
                                    orbital_loss.py; no reference code, tested against numpy, torch autograd and the solver route)
  nabladft_amd.purified_occupied_energies / OccupiedEnergyLoss / OccupiedOrbitals / PurifiedOrbitalErrors / QHNetPurifiedOrbitalLightning <-> the same slots, for
                                    ALL occupied levels and coefficients: a pivoted Cholesky factor of the purified projector and an n_occ x n_occ solve
                                    (orbitals.py, orbital_loss.py; no reference code, tested against numpy, scipy, torch autograd and the solver route)
  nabladft_amd.spk.*            <-> the schnetpack classes config/model/{painn,schnet}.yaml instantiate (parity unpinned)
  nabladft_amd.read_energy_database / ArenaLoader <-> PyGNablaDFT.process + DataLoader collate (dataset/pyg_datasets.py:101-109)
"""
from .painn import PaiNN, NeighborList, build_neighbor_list  # noqa: F401
from .lightning import AtomisticTaskFixed, EquiformerV2_OC20_Lightning, GemNetOCLightning, eSCNLightning, L2Loss, ModelOutput, PaiNNLightning, QHNetLightning  # noqa: F401
from .qhnet import QHNet  # noqa: F401
from .gemnet_oc import GemNetOC  # noqa: F401
from .escn import eSCN  # noqa: F401
from .equiformer_v2 import EquiformerV2_OC20  # noqa: F401
from .graphormer import Graphormer3D, Graphormer3DLightning  # noqa: F401
from .dimenetplusplus import DimeNetPlusPlusForceLightning, DimeNetPlusPlusLightning, DimeNetPlusPlusPotential  # noqa: F401
from . import ema, schedulers  # noqa: F401
from .trainer import FusedTrainStep, Batch  # noqa: F401
from . import optimization  # noqa: F401
from .optimization import ASEBatchwiseLBFGS, BatchwiseOptimizeTask, PyGBatchwiseCalculator  # noqa: F401
from . import md  # noqa: F401
from .md import BatchedMD, PYGAseInterface  # noqa: F401
from . import vibrations  # noqa: F401
from .vibrations import BatchedVibrations  # noqa: F401
from . import orbitals  # noqa: F401
from .orbitals import BatchedOrbitals, BatchedPurification, FermiResult, OrbitalErrors, OrbitalState, electron_counts, mulliken_charges, occupied_counts, bond_layout, dense_bond_orders, LowdinBasis, BatchedMatrixRoot, ScfResidualErrors, FrontierLevels, OccupiedOrbitals, PurifiedOrbitalErrors  # noqa: F401
from .orbital_loss import (DensityMatrixLoss, MullikenChargeLoss, OrbitalEnergyLoss, QHNetDensityLightning, QHNetOrbitalLightning,  # noqa: F401
                           QHNetSmearedDensityLightning, SmearedSolution, density_matrix, orbital_energies, orbital_solution, populations,
                           smeared_density_matrix, smeared_solution, purified_density_matrix, QHNetPurifiedDensityLightning, bond_orders, BondOrderLoss,
                           QHNetBondOrderLightning, lowdin_basis, lowdin_density, lowdin_hamiltonian, lowdin_populations, lowdin_charges, lowdin_bond_orders,
                           LowdinChargeLoss, QHNetLowdinLightning, commutator, scf_residual, scf_residual_to_target, ScfResidualLoss, ScfTarget, scf_target,
                           scf_target_iterative, scf_target_blocks, QHNetCommutatorLightning, purified_frontier, FrontierLoss, QHNetPurifiedFrontierLightning,
                           purified_occupied_energies, OccupiedEnergyLoss, QHNetPurifiedOrbitalLightning)
from .data import ArenaLoader, ConformerArena, HamiltonianBatch, HamiltonianDatabase, HamiltonianDataset, hamiltonian_batch, read_energy_database  # noqa: F401

__all__ = ["PaiNN", "PaiNNLightning", "QHNet", "QHNetLightning", "GemNetOC", "GemNetOCLightning", "eSCN", "eSCNLightning", "EquiformerV2_OC20", "EquiformerV2_OC20_Lightning", "Graphormer3D", "Graphormer3DLightning", "DimeNetPlusPlusPotential", "DimeNetPlusPlusLightning", "DimeNetPlusPlusForceLightning", "AtomisticTaskFixed", "ModelOutput", "L2Loss", "FusedTrainStep", "Batch", "build_neighbor_list", "NeighborList", "ArenaLoader", "ConformerArena",
           "read_energy_database", "HamiltonianDatabase", "HamiltonianDataset", "HamiltonianBatch", "hamiltonian_batch", "ASEBatchwiseLBFGS", "PyGBatchwiseCalculator", "BatchwiseOptimizeTask", "BatchedMD", "BatchedVibrations", "PYGAseInterface", "BatchedOrbitals", "OrbitalState", "OrbitalErrors", "orbital_energies", "OrbitalEnergyLoss", "QHNetOrbitalLightning", "mulliken_charges", "occupied_counts", "orbital_solution", "density_matrix", "populations", "DensityMatrixLoss", "MullikenChargeLoss", "QHNetDensityLightning", "electron_counts", "FermiResult", "SmearedSolution", "smeared_solution", "smeared_density_matrix", "QHNetSmearedDensityLightning", "BatchedPurification", "purified_density_matrix", "QHNetPurifiedDensityLightning", "bond_orders", "BondOrderLoss", "QHNetBondOrderLightning",
           "bond_layout", "dense_bond_orders", "LowdinBasis", "lowdin_basis", "lowdin_density", "lowdin_hamiltonian", "lowdin_populations", "lowdin_charges",
           "lowdin_bond_orders", "LowdinChargeLoss", "QHNetLowdinLightning", "commutator", "scf_residual", "scf_residual_to_target", "ScfResidualLoss", "ScfTarget",
           "scf_target", "scf_target_iterative", "scf_target_blocks", "BatchedMatrixRoot", "QHNetCommutatorLightning", "ScfResidualErrors", "purified_frontier", "FrontierLoss",
           "FrontierLevels", "QHNetPurifiedFrontierLightning", "purified_occupied_energies", "OccupiedEnergyLoss", "QHNetPurifiedOrbitalLightning", "OccupiedOrbitals",
           "PurifiedOrbitalErrors"]
