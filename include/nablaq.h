/* nablaq.h -- C ABI of libnablaq.so, the MI355X (gfx950) engine for the nablaDFT PaiNN hot path.
 *
 * Drop-in boundary.  The reference is pure Python; its "FFI" for this path is the set
 * of third-party native ops it calls from nablaDFT/painn_pyg (paths relative to /root/reference/):
 *
 *   nq_graph_count / nq_graph_fill   replace torch_cluster.radius_graph (painn.py:411-416), the edge
 *                                    geometry (painn.py:418-423, :319-321), compute_neighbors
 *                                    (utils.py:469-481) and symmetrize_edges (painn.py:168-304)
 *   nq_painn_forward                 replaces PaiNN.forward (painn.py:89-148): RadialBasis
 *                                    (layers.py:181-185), AtomEmbedding (layers.py:215-222), 6x
 *                                    PaiNNMessage (painn.py:475-509; PyG propagate + torch_scatter.scatter)
 *                                    and PaiNNUpdate (painn.py:535-548), out_energy + scatter
 *                                    (painn.py:127-128) and forces = -autograd.grad (painn.py:135-146)
 *   nq_painn_backward                replaces loss.backward() through the create_graph=True force graph
 *                                    (painn.py:142; Lightning backward after painn.py:655-668)
 *   nq_loss_l1_l2                    replaces _calculate_loss (painn.py:741-745) with L1Loss + L2Loss
 *                                    (gemnet_oc/loss.py:5-22; config/model/painn-oc.yaml:36-43)
 *   nq_adamw_step                    replaces clip_grad_norm (config/painn-oc.yaml:18-19) + torch.optim.AdamW
 *
 * Conventions: every pointer is a DEVICE pointer owned by the caller (torch tensors) unless it is
 * named *_host; all arrays are contiguous row-major fp32 / int32 / int64 as stated; `stream` is a
 * hipStream_t passed as void*; functions are re-entrant (no global mutable state except the
 * thread-local error string); return value 0 = NQ_OK, otherwise an NQ_ERR_* code and
 * nq_last_error() describes it.  Nothing here allocates device memory.
 */
#ifndef NABLAQ_H
#define NABLAQ_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NQ_OK 0
#define NQ_ERR_HIP 1
#define NQ_ERR_ARG 2
#define NQ_ERR_MOL_TOO_LARGE 3
#define NQ_ERR_WORKSPACE 4
#define NQ_ERR_NO_EDGES 5

#define NQ_ABI_VERSION 17

/* Model hyper-parameters = constructor arguments of nablaDFT.painn_pyg.PaiNN (painn.py:28-45). */
typedef struct nq_painn_cfg {
  int32_t hidden_channels;   /* F, multiple of 64, <= 1024 */
  int32_t num_layers;        /* L */
  int32_t num_rbf;           /* R */
  int32_t num_elements;      /* rows of atom_emb.embeddings.weight */
  int32_t max_neighbors;     /* K of radius_graph */
  int32_t envelope_exponent; /* PolynomialEnvelope(exponent) (layers.py:14-33); 0 selects ExponentialEnvelope (layers.py:36-48) */
  double cutoff;             /* Angstrom */
  float rbf_coeff;           /* GaussianSmearing.coeff = -0.5/(offset[1]-offset[0])^2 */
  int32_t filter_mode;       /* 0: painn_pyg  filter = rbf_proj(envelope(d/rc) * gauss(d/rc)) + bias   (layers.py:181-185)
                              * 1: schnetpack filter = cosine_cutoff(d) * (filter_net(gauss(d)) + bias), Gaussians on the unscaled
                              *    distance (config/model/painn.yaml:9-16); needs the fused-filter path */
  int32_t rbf_type;          /* RadialBasis(rbf=...) (layers.py:168-179): 0 gaussian; 1 spherical_bessel (learnable frequencies [R]);
                              * 2 bernstein (learnable pregamma).  1 and 2 use the materialised-filter path; their parameters sit in the
                              * flat buffer right after atom_emb.embeddings.weight (state_dict order); for 2 `rbf_offsets` carries the
                              * BernsteinBasis.prefactor buffer (binomial coefficients). */
  int32_t reserved;
} nq_painn_cfg;

/* Neighbour list in engine layout (CSR by target atom, sources ascending; symmetric). */
typedef struct nq_graph {
  int32_t N, B, E;
  int32_t max_mol_atoms;    /* largest molecule of the batch (the value passed to nq_graph_count); 0 = unknown: the per-molecule LDS kernels
                             * (rbf_proj gradient with node rows staged per molecule, csrc/molpair.hip) are then replaced by the row-gather path */
  const int32_t* mol_ptr;   /* [B+1] first atom of each molecule */
  const int32_t* row_ptr;   /* [N+1] */
  const int32_t* col;       /* [E] source atom of the in-edge at this slot */
  const int32_t* dst;       /* [E] target atom of the slot (row index) */
  const int32_t* rev;       /* [E] slot of the reverse edge */
  const float* geom;        /* [E][4] {rx, ry, rz, d}, r = (pos[col]-pos[dst])/d */
  const int32_t* z;         /* [N] atomic numbers */
  const int32_t* atom_mol;  /* [N] molecule of each atom */
  const int32_t* lowptr;    /* [N+1] prefix count of in-edges with source < target (the first entries of each row); output of
                             * nq_graph_count.  Numbers the undirected pairs: pair(i <- j, j < i) = lowptr[i] + position in row i. */
} nq_graph;

int nq_abi_version(void);
const char* nq_last_error(void);

/* ---- neighbour list ------------------------------------------------------------------------ */
/* Pass 1: degrees and prefix sums; returns the number of directed edges E in *E_host (synchronises
 * `stream`).  deg/lowdeg: int32[N] scratch; row_ptr/lowptr: int32[N+1] outputs. */
int nq_graph_count(const float* pos, const int32_t* mol_ptr, int32_t N, int32_t B, int32_t max_mol_atoms, double cutoff,
                   int32_t max_neighbors, int32_t* deg, int32_t* lowdeg, int32_t* row_ptr, int32_t* lowptr, int32_t* E_host,
                   void* stream);
/* Pass 2: fills the CSR arrays (col, dst, rev, geom[E][4], slot2canon, atom_mol[N]) and, if edge_index != NULL,
 * the reference's canonical outputs: edge_index int64[2][E] (row0 = source j, row1 = target i),
 * edge_dist f32[E], edge_vector f32[E][3], id_swap int64[E], neighbors int64[B].  E == 0 (no pair inside the cutoff): the per-slot
 * arrays may be NULL, atom_mol and neighbors are still written.  max_mol_atoms above the limit of nq_graph_count: NQ_ERR_MOL_TOO_LARGE. */
int nq_graph_fill(const float* pos, const int32_t* mol_ptr, int32_t N, int32_t B, int32_t E, int32_t max_mol_atoms, double cutoff,
                  int32_t max_neighbors, const int32_t* row_ptr, const int32_t* lowptr, int32_t* col, int32_t* dst, int32_t* rev,
                  float* geom, int32_t* slot2canon, int32_t* atom_mol, int64_t* edge_index, float* edge_dist, float* edge_vector,
                  int64_t* id_swap, int64_t* neighbors, void* stream);

/* ---- model --------------------------------------------------------------------------------- */
/* Flat parameter buffer: tensors concatenated in state_dict order of the reference PaiNN
 * (atom_emb.embeddings.weight, message_layers.{l}.{x_proj.0,x_proj.2,rbf_proj}.{weight,bias} for all l,
 * update_layers.{l}.{vec_proj.weight, xvec_proj.0.{weight,bias}, xvec_proj.2.{weight,bias}} for all l,
 * out_energy.{0,2}.{weight,bias}). */
size_t nq_painn_num_params(const nq_painn_cfg* cfg);
size_t nq_painn_workspace_bytes(const nq_painn_cfg* cfg, int32_t N, int32_t E, int32_t B);

/* energy[B] and (if forces != NULL) forces[N][3] = -dE_tot/dpos.  Keeps every activation in `workspace`
 * for nq_painn_backward -- and, when forces are computed, the per-layer adjoints of that force sweep: they are the
 * tangent adjoints of the second-order sweep, which nq_painn_backward reads instead of recomputing (same parameters
 * required in both calls, as before).  rbf_offsets: f32[R] = buffer radial_basis.rbf.offset. */
int nq_painn_forward(const nq_painn_cfg* cfg, const float* params, const float* rbf_offsets, const nq_graph* graph, void* workspace,
                     size_t workspace_bytes, float* energy, float* forces, void* stream);
/* Given dL/dE[B] and dL/dF[N][3] (either may be NULL = zeros) writes dL/dparams[num_params] (overwrites).
 * Must follow nq_painn_forward on the same workspace and graph; after a forward call without forces (energy-only training) it runs the full
 * dual sweep instead of reading the stored force-sweep adjoints.
 * The workspace layout and every path choice (fused filter, rbf_proj gradient path, stored adjoints) are the ones the last forward call on
 * this workspace made; environment switches changed after it have no effect.  Returns NQ_ERR_ARG before any device work when no forward call
 * has prepared the workspace, or when that call was made for another nq_painn_cfg or another batch (N, E, B, max_mol_atoms).
 * The same holds for nq_painn_backward_events and nq_painn_backward_seeded. */
int nq_painn_backward(const nq_painn_cfg* cfg, const float* params, const float* rbf_offsets, const nq_graph* graph, void* workspace,
                      size_t workspace_bytes, const float* grad_energy, const float* grad_forces, float* grad_params, void* stream);
/* nq_painn_backward with completion events: layer_events_host[i] (HOST array of L hipEvent_t, entries may be NULL) is recorded on `stream` as soon as
 * every gradient slice of layer L-1-i is final (the reverse sweep runs from the last layer to the first; the read-out head's slices are final with
 * event 0, the embedding's when the call's work is complete), so that a data-parallel caller can all-reduce finished slices on a side stream while the
 * earlier layers are still being differentiated (reference: torch DDP's bucketed all-reduce under Lightning's DDPStrategy, utils/pipelines.py:65-68).
 * nq_painn_layer_param_ranges: ranges_host int64[4 (L+1)] = per layer {message offset, count, update offset, count} in floats of the flat buffer,
 * then {head offset, count, embedding offset, count}. */
int nq_painn_backward_events(const nq_painn_cfg* cfg, const float* params, const float* rbf_offsets, const nq_graph* graph, void* workspace,
                             size_t workspace_bytes, const float* grad_energy, const float* grad_forces, float* grad_params, void* const* layer_events_host,
                             void* stream);
int nq_painn_layer_param_ranges(const nq_painn_cfg* cfg, int64_t* ranges_host);
/* First-order reverse for the direct-force model (direct_forces=True, painn.py:130-133; the PaiNNOutput head itself, painn.py:551-620, is
 * evaluated by the caller on the final node state "x_in"/"vec_in" at layer L of the workspace): given dL/dE[B] and the adjoints of the
 * final x [N][F] and vec [N][3][F] (any may be NULL) writes dL/dparams.  Must follow nq_painn_forward (forces == NULL) on the same workspace. */
int nq_painn_backward_seeded(const nq_painn_cfg* cfg, const float* params, const float* rbf_offsets, const nq_graph* graph, void* workspace,
                             size_t workspace_bytes, const float* grad_energy, const float* grad_x, const float* grad_vec, float* grad_params,
                             void* stream);
/* Elementwise pieces of GatedEquivariantBlock (painn.py:583-620), the GEMMs in between are nq_linear_*:
 * nq_scaled_silu: out = silu(z)/0.6 (grad_y == NULL) or grad_y * dsilu(z)/0.6;  nq_geb_cat: cat[N][2h] = [x | ||v1||_xyz], v1 [N][3][h];
 * nq_geb_gate: (xo | gate) = split(o2 [N][2o]); xout = ScaledSiLU(xo), vout [N][3][o] = gate * v2. */
int nq_scaled_silu(const float* z, const float* grad_y, float* out, int64_t count, void* stream);
int nq_geb_cat(const float* x, const float* v1, int64_t N, int32_t h, float* cat, void* stream);
int nq_geb_cat_backward(const float* grad_cat, const float* v1, int64_t N, int32_t h, float* grad_x, float* grad_v1, void* stream);
int nq_geb_gate(const float* o2, const float* v2, int64_t N, int32_t o, float* xout, float* vout, void* stream);
int nq_geb_gate_backward(const float* o2, const float* v2, const float* grad_xout, const float* grad_vout, int64_t N, int32_t o, float* grad_o2,
                         float* grad_v2, void* stream);
/* Largest molecule (atoms) whose rbf_proj gradient runs on the per-molecule LDS kernel (csrc/molpair.hip): its 20 rows of a 32-channel slice must fit one
 * workgroup's LDS.  Larger molecules of a batch take the pair-row kernels, the rest of the batch is not affected (painn.py:475-509 semantics either way). */
int32_t nq_painn_molecule_lds_atoms(void);
/* Test/inspection hook: offset (in floats) and element count of a named workspace buffer, e.g.
 * ("x_msg", 2, tangent=0).  Returns NQ_ERR_ARG for unknown names. */
int nq_painn_ws_lookup(const nq_painn_cfg* cfg, int32_t N, int32_t E, int32_t B, const char* name, int32_t layer, int32_t tangent,
                       size_t* offset_floats, size_t* count);

/* ---- SchNet (schnetpack 2.0.4 representation.SchNet + Atomwise + Forces as instantiated by config/model/schnet.yaml:4-28;
 *      third-party arithmetic, PARITY UNPINNED -- oracle/spk_schnet_ref.py) -------------------------------------------------- */
typedef struct nq_schnet_cfg {
  int32_t n_atom_basis;    /* F in {64,128,256} (n_filters = n_atom_basis) */
  int32_t n_interactions;  /* L */
  int32_t n_rbf;           /* GaussianRBF(n_rbf, cutoff): 2 <= n_rbf <= 268 (the k0 sort of the first-layer weight gradient has 256 bins:
                            * n_rbf - min(n_rbf, 13) + 1 <= 256) and max(n_rbf, 13) * F * 4 B <= 156 KB (W1^T in LDS: 156 at F = 256); anything
                            * else is refused with NQ_ERR_ARG before any device work */
  int32_t max_z;           /* rows of representation.embedding.weight (row 0 = padding) */
  double cutoff;           /* CosineCutoff(cutoff) = GaussianRBF cutoff, Angstrom */
  float rbf_coeff;         /* -0.5 / width^2, width = offsets[1] - offsets[0] */
  int32_t reserved;
} nq_schnet_cfg;
/* Flat parameter buffer = the tensors in module order: representation.embedding.weight [max_z][F]; per interaction l:
 * in2f.weight [F][F], filter_network.{0.weight [F][R], 0.bias, 1.weight [F][F], 1.bias}, f2out.{0.weight, 0.bias, 1.weight, 1.bias};
 * output_modules.0.outnet.{0.weight [F/2][F], 0.bias, 1.weight [1][F/2], 1.bias}. */
size_t nq_schnet_num_params(const nq_schnet_cfg* cfg);
size_t nq_schnet_workspace_bytes(const nq_schnet_cfg* cfg, int32_t N, int32_t E, int32_t B);
/* Same contracts as nq_painn_forward / nq_painn_backward; rbf_offsets = GaussianRBF.offsets f32[n_rbf] (unscaled distances);
 * the graph is the full list inside the cutoff (nq_graph_count/fill with max_neighbors >= molecule size). */
int nq_schnet_forward(const nq_schnet_cfg* cfg, const float* params, const float* rbf_offsets, const nq_graph* graph, void* workspace,
                      size_t workspace_bytes, float* energy, float* forces, void* stream);
int nq_schnet_backward(const nq_schnet_cfg* cfg, const float* params, const float* rbf_offsets, const nq_graph* graph, void* workspace,
                       size_t workspace_bytes, const float* grad_energy, const float* grad_forces, float* grad_params, void* stream);
/* Test/inspection hook like nq_painn_ws_lookup: offset (in floats) and element count of a named buffer of the SchNet workspace; host-only arithmetic.
 * Buffer names are those of oracle/spk_schnet_ref.py:SchNetSweeps; P = E/2 undirected pairs; tangent = 1 selects the tangent half where one exists.
 *   per layer, with a tangent half: "x" (layers 0..L), "y", "m", "t1", "u" [N][F]; "a1", "h2" [P][F];  "zo" [N][F/2] (with tangent half);
 *   "e_atom", "te_atom" [N];  "rw" [P][32] window records, "order" [P] / "pair_of" [E] / "pair_slot" [P] (int32 payloads), "geomp" [P][4];
 *   "td" [E] (per slot), "tdp" [P], "gd_total" [P] (dE/dd summed over the layers and both directed edges, after a forward call with forces);
 *   the adjoint buffers SHARED by all layers "gx", "gu", "gm", "gy" [2][N][F] and "gh2", "ga1" [2][P][F]: after nq_schnet_backward they hold the
 *   layer processed last, layer 0 ("gu" = (gt1, gtt1), "ga1" = (gz1, gtz1 * td) -- the in-place results; "gx" = the adjoints of x[0]).
 * NQ_ERR_ARG with a message for an unknown name, a layer out of range, or a tangent half asked of a buffer that has none. */
int nq_schnet_ws_lookup(const nq_schnet_cfg* cfg, int32_t N, int32_t E, int32_t B, const char* name, int32_t layer, int32_t tangent,
                        size_t* offset_floats, size_t* count);

/* ---- Hamiltonian block assembly (QHNet.build_final_matrix, qhnet/qhnet.py:293-321; + H + H^T, qhnet.py:237; HamiltonianLoss,
 *      qhnet/loss.py:9-16).  Packed result layout: molecule after molecule, M_b x M_b row-major, M_b = orbitals of molecule b;
 *      pack_ptr[b] = sum_{b' < b} M_b'^2, mol_orb_ptr[b] = sum_{b' < b} M_b'.  All index arrays are device pointers. ------------- */
/* Tables for one batch: orb_atom / orb_slot [sum M_b] (global orbital -> atom, slot of the padded S x S block = mask[Z][t], the table
 * of QHNet._get_mask, qhnet.py:323-342), look [sum_b n_b^2] (ordered atom pair -> index into the pair-block array; e_dst = row 0 and
 * e_src = row 1 of data.full_edge_index, qhnet.py:296).  orb_ptr [N+1]: prefix of mask_count[z]; pair_base [B]: prefix of n_b^2.
 * err_flag (device int32) becomes non-zero if a pair joins two molecules (1) or, later, a needed pair is missing (2). */
int nq_hblock_tables(const int32_t* z, const int32_t* atom_mol, const int32_t* mol_ptr, int32_t N, int32_t B, const int64_t* orb_ptr,
                     const int64_t* pair_base, const int64_t* e_dst, const int64_t* e_src, int64_t P, const int32_t* mask_table,
                     const int32_t* mask_count, int32_t S, int32_t* orb_atom, int32_t* orb_slot, int32_t* look, int64_t look_count,
                     int32_t* err_flag, void* stream);
/* out_packed[total]: block (dst rows, src columns) = diag[atom] or nondiag[pair(dst, src)] on the atoms' orbital slots; symmetrize != 0
 * adds the transposed element (H + H^T).  diag is [N][S][S] and nondiag [P][S][S] with the N and P the tables were built for; this call
 * is given neither, so the caller answers for both sizes (BlockAssembler.assemble checks them); nondiag may be NULL only where P = 0. */
int nq_hblock_assemble(const float* diag, const float* nondiag, const int32_t* mol_ptr, const int64_t* pair_base, const int64_t* pack_ptr,
                       const int64_t* mol_orb_ptr, const int32_t* orb_atom, const int32_t* orb_slot, const int32_t* look, int32_t B, int32_t S,
                       int32_t symmetrize, int64_t total, float* out_packed, int32_t* err_flag, void* stream);
/* Reverse of nq_hblock_assemble: grad_diag [N][S][S], grad_nondiag [P][S][S] (unused slots get 0).  inv_table [Zt][S]: slot -> local
 * orbital of that atom type or -1.  With P > 0 a NULL e_dst, e_src or grad_nondiag is refused (NQ_ERR_ARG). */
int nq_hblock_assemble_backward(const float* grad_packed, const int32_t* z, const int32_t* atom_mol, const int64_t* orb_ptr, const int64_t* pack_ptr,
                                const int64_t* mol_orb_ptr, const int32_t* inv_table, const int64_t* e_dst, const int64_t* e_src, int32_t N,
                                int64_t P, int32_t S, int32_t symmetrize, float* grad_diag, float* grad_nondiag, void* stream);
/* to_dense != 0: dense [m_total][m_total] = block_diag of the packed blocks (zero elsewhere; what the reference returns);
 * to_dense == 0: packed <- the diagonal blocks of dense. */
int nq_hblock_packed_dense(float* packed, float* dense, const int64_t* pack_ptr, const int64_t* mol_orb_ptr, int32_t B, int64_t total, int64_t m_total,
                           int32_t to_dense, void* stream);
/* PhiSNet irreps -> matrix (NeuralNetwork.matrix_block / generate_matrix_from_irreps + the collection loops of forward,
 * phisnet/nn/neural_network.py:636-706, 859-918): packed result as above; block(i,j)[(n_i,m_i),(n_j,m_j)] =
 * sum_L sum_M cg_table[l_i][l_j][L][m_i][m_j][M] * f[row][L*L+M][idx(type_i, type_j, n_i, n_j, L)], f = f_ii[atom] or f_ij[pair(i, j)]
 * ([rows][ncomp][Fo]); cg_table [3][3][5][5][5][9] = sqrt(2L+1) * the model's Clebsch-Gordan tensors; shell tables [T][32]; idx_ii
 * [T][S][S][5], idx_ij [T][T][S][S][5] (-1 = absent).  orb_local: local orbital index inside its atom (nq_hblock_tables with identity masks).
 * unit_diagonal: overlap matrices (diagonal = 1, neural_network.py:964-965).  Backward: inv_ii [T][5][Fo], inv_ij [T][T][5][Fo] = n_i*S+n_j or -1.
 * f_ii and f_ij share ncomp and Fo: Fo exceeds every index held in idx_ii / idx_ij and ncomp reaches (L+1)^2 of the highest L they carry (the caller
 * pads the narrower tensor; IrrepsAssembler.assemble checks all of it).  Backward refuses a NULL e_i, e_j or grad_f_ij where P > 0 (NQ_ERR_ARG). */
int nq_irreps_assemble(const float* f_ii, const float* f_ij, const int32_t* z, const int32_t* mol_ptr, const int64_t* pair_base, const int64_t* pack_ptr,
                       const int64_t* mol_orb_ptr, const int64_t* orb_ptr, const int32_t* orb_atom, const int32_t* orb_local, const int32_t* look,
                       int32_t B, int32_t ncomp, int32_t Fo, const int32_t* tz, const int32_t* sh_n, const int32_t* sh_l, const int32_t* sh_m,
                       const int32_t* sh_off, const int32_t* idx_ii, const int32_t* idx_ij, const float* cg_table, int32_t T, int32_t S,
                       int32_t symmetrize, int32_t unit_diagonal, int64_t total, float* out_packed, int32_t* err_flag, void* stream);
int nq_irreps_assemble_backward(const float* grad_packed, const int32_t* z, const int32_t* atom_mol, const int64_t* e_i, const int64_t* e_j,
                                const int64_t* pack_ptr, const int64_t* mol_orb_ptr, const int64_t* orb_ptr, const int32_t* inv_ii, const int32_t* inv_ij,
                                int64_t N, int64_t P, int32_t ncomp, int32_t Fo, const int32_t* tz, const int32_t* sh_n, const int32_t* sh_l,
                                const int32_t* sh_m, const int32_t* sh_off, const float* cg_table, int32_t T, int32_t S, int32_t symmetrize,
                                int32_t unit_diagonal, float* grad_f_ii, float* grad_f_ij, void* stream);
/* stats3 = {loss = sqrt(sum d^2 / total) + sum|d| / total, rmse, sum|d|} (mask.sum() == total for block-diagonal targets);
 * grad_packed (nullable) = grad_scale * dloss/dpred.  scratch: 512 doubles. */
int nq_hamiltonian_loss(const float* pred_packed, const float* target_packed, int64_t total, float grad_scale, float* stats3, float* grad_packed,
                        double* scratch, void* stream);

/* ---- SO(3) Clebsch-Gordan mixing (PhiSNet PairMixing / SelfMixing contraction: phisnet/nn/modules/pair_mixing.py:47-69,
 *      self_mixing.py:55-83).  x1 [rows][(order1+1)^2][F], x2 [rows][(order2+1)^2][F], y [rows][(order_out+1)^2][F], orders <= 4,
 *      components of all orders concatenated (offset l*l + m + l).  path_index_host: HOST int8[65], for every path (l1,l2,L) in the
 *      loop order of PairMixing.forward over orders 4/4/4 the index of its coefficient among the enabled paths, or -1.
 *      coeff [rows][n_enabled][F] (coeff_row_stride = n_enabled*F) or [n_enabled][F] shared by all rows (coeff_row_stride = 0).
 *      keep (nullable) [keep_orders][F]: y_L += keep_L * x1_L.  The kernels use the canonical tensors of nabladft_amd/cg.py; a model's
 *      own sign convention is folded into coeff by the caller. ------------------------------------------------------------------ */
int nq_so3_mix_forward(const float* x1, const float* x2, const float* coeff, const float* keep, int64_t rows, int32_t F, int32_t order1,
                       int32_t order2, int32_t order_out, const int8_t* path_index_host, int64_t coeff_row_stride, int32_t keep_orders, float* y,
                       void* stream);
/* grad_coeff_rows [rows][n_enabled][F] and grad_keep_rows [rows][keep_orders][F] are per-row contributions (sum over rows for shared
 * coefficients); grad_x1 / grad_x2 have the shapes of x1 / x2 (for x1 == x2 add them). */
int nq_so3_mix_backward(const float* x1, const float* x2, const float* coeff, const float* keep, const float* grad_y, int64_t rows, int32_t F,
                        int32_t order1, int32_t order2, int32_t order_out, const int8_t* path_index_host, int64_t coeff_row_stride,
                        int32_t keep_orders, float* grad_x1, float* grad_x2, float* grad_coeff_rows, float* grad_keep_rows, void* stream);

/* The same reverse pass for coefficients SHARED by all rows (SelfMixing; QHNet's SelfNetLayer): dL/dcoeff is reduced over rows inside the kernel;
 * grad_coeff_partials [nq_so3_mix_partial_blocks(rows, F)][n_enabled][F] are per-workgroup partial sums (sum them in order for the result).
 * F must divide 256. */
int64_t nq_so3_mix_partial_blocks(int64_t rows, int32_t F);
int nq_so3_mix_backward_shared(const float* x1, const float* x2, const float* coeff, const float* keep, const float* grad_y, int64_t rows, int32_t F,
                               int32_t order1, int32_t order2, int32_t order_out, const int8_t* path_index_host, int32_t keep_orders, float* grad_x1,
                               float* grad_x2, float* grad_coeff_partials, float* grad_keep_rows, void* stream);

/* ---- QHNet SO(3) tensor-product layers (nablaDFT/qhnet/layers.py; e3nn 0.5.1 TensorProduct / Linear / Norm semantics restated in
 *      oracle/e3nn_mini.py, PARITY UNPINNED for the e3nn part).  Irreps features are [rows][(lmax+1)^2][C], component l*l + m + l, channel
 *      fastest.  Graph arrays (int32, device): row_ptr [N+1] CSR by owner atom = "src" = row 1 of the reference's edge_index (qhnet.py:262),
 *      col [R] = "dst" = row 0 ascending, own [R] = owner of each slot, rev [R] = slot of the reverse edge (the neighbour relation is
 *      symmetric).  Path weights carry e3nn's sign and path normalisation (folded in by the caller). ------------------------------------------------------------------------------------- */
/* s0 [R][(2+lmax) C] = [x_0[dst] | x_0[dst] (conv, layers.py:240-246) or x_0[src] (pair, layers.py:469-475) | <x_l[dst], x_l[src]>/(2l+1)]
 * = InnerProduct (layers.py:277-294) + the concatenations of ConvLayer.forward / PairNetLayer.forward. */
int nq_qh_invariants_forward(const float* x, int64_t N, int32_t ncomp, int32_t C, const int32_t* own, const int32_t* col, int64_t R,
                             int32_t second_from_owner, float* s0, void* stream);
int nq_qh_invariants_backward(const float* x, const float* grad_s0, int64_t N, int32_t ncomp, int32_t C, const int32_t* row_ptr, const int32_t* col,
                              const int32_t* rev, int32_t second_from_owner, float* grad_x, void* stream);
/* Tensor products per row (edge or ordered pair), the arithmetic of e3nn's TensorProduct in QHNet:
 *   sh != NULL ('uvu', ConvLayer.tp_node, layers.py:262): y[r] = sum_paths w1 w2 CG . x[idx1[r]] . sh[r];  sh [R][25] real spherical harmonics of
 *       pos[dst] - pos[src];  path_set 1 = the 42 paths with even l1+l2+L (x [N][25][C]), 2 = the 5 paths of the first layer (x [N][1][C]);
 *   sh == NULL ('uuu', PairNetLayer.tp_node_pair, layers.py:481): second operand x[idx2[r]]; path_set 0 = all 65 paths.
 * w1, w2 (nullable second factor, multiplied in-kernel): [R][nq_qh_tp_num_paths(path_set)][C] in e3nn instruction order.  y_rows [R][25][C].
 * Backward: grad_y rows are read at idx_gy[r] (NULL = r); per-row operand adjoints grad_x1_rows [R][ncomp1][C], grad_x2_rows [R][25][C]
 * (uuu only) are summed over each atom's rows by nq_qh_pair_reduce; grad_w1 / grad_w2 like w1 / w2. */
/* 'uuu' forward with the two weight factors generated inside the kernel (csrc/qhgen.hip; layers.py:476-481: weight = fc_node_pair(edge_attr) * fc(s0)):
 *   w1[r] = h1[r] W1 (* col_scale), w2[r] = h2[r] W2^T + bias2, h1 / h2 [R][K] the hidden activations of the two generators (K = 32 / 64 / 128).
 * nq_qh_gen_presplit turns a generator's last weight matrix (layout 0: [K][65 C] as x @ W; 1: [65 C][K] as nn.Linear) into nq_qh_gen_fragment_floats(C, K)
 * floats of bf16 matrix-instruction fragments, once per optimiser step.  The weight factors never exist in HBM; nq_qh_tp_backward_gen is the reverse sweep with the same
 * in-kernel generation (it returns the adjoints of both factors, [R][65][C] each: the operands of the generators' own weight gradients). */
size_t nq_qh_gen_fragment_floats(int32_t C, int32_t K);
int nq_qh_gen_presplit(const float* W, const float* col_scale, int32_t K, int32_t C, int32_t layout, float* fragments, void* stream);
int nq_qh_tp_forward_gen(const float* x, const int32_t* idx1, const int32_t* idx2, const float* h1, const float* h2, const float* frag1, const float* frag2,
                         const float* bias2, int64_t R, int32_t C, int32_t K, float* y_rows, void* stream);
int nq_qh_tp_backward_gen(const float* x, const int32_t* idx1, const int32_t* idx2, const float* h1, const float* h2, const float* frag1, const float* frag2,
                          const float* bias2, const float* grad_y, int64_t R, int32_t C, int32_t K, float* grad_x1_rows, float* grad_x2_rows, float* grad_w1,
                          float* grad_w2, void* stream);
int nq_qh_tp_num_paths(int32_t path_set);
void nq_qh_set_tp_variant(int32_t variant);   /* tuning hook (process-global): 0 per-path weight loads, 1 / 2 chunked prefetch with / without scheduling barriers */
int nq_qh_tp_forward(const float* x, int32_t ncomp1, const int32_t* idx1, const float* sh, const int32_t* idx2, const float* w1, const float* w2, int64_t R,
                     int32_t C, int32_t path_set, float* y_rows, void* stream);
int nq_qh_tp_backward(const float* x, int32_t ncomp1, const int32_t* idx1, const float* sh, const int32_t* idx2, const float* w1, const float* w2,
                      const float* grad_y, const int32_t* idx_gy, int64_t R, int32_t C, int32_t path_set, float* grad_x1_rows, float* grad_x2_rows,
                      float* grad_w1, float* grad_w2, void* stream);
/* out[n][k] = base[n][k] + sum_{r in row n} (rows_own[r][k] + rows_nbr[rev[r]][k]), k < width (each operand may be NULL = zeros): the scatter of
 * ConvLayer (torch_scatter.scatter, layers.py:268: messages arrive along the reverse slots of the receiver's own row) and the reverse of every
 * per-row gather; fixed order, no atomics. */
int nq_qh_pair_reduce(const float* rows_own, const float* rows_nbr, const float* base, const int32_t* row_ptr, const int32_t* rev, int64_t N, int32_t width,
                      float* out, void* stream);
/* NormGate pieces (layers.py:141-147; e3nn o3.Norm + ElementwiseTensorProduct): nq_qh_normcat: out [rows][(lmax+1) C] = [x_0 | ||x_1|| | ...]
 * (grad_f0 == NULL) or the adjoint of x [rows][ncomp][C] given grad_f0;  nq_qh_gate: y = [gates_0 | x_l * gates_l] (grad_y == NULL) or
 * (grad_x, grad_gates) given grad_y. */
int nq_qh_normcat(const float* x, const float* grad_f0, int64_t rows, int32_t C, int32_t lmax, float* out, void* stream);
int nq_qh_gate(const float* x, const float* gates, const float* grad_y, int64_t rows, int32_t C, int32_t lmax, float* y, float* grad_x, float* grad_gates,
               void* stream);
/* out = cst * act(x) (grad_y == NULL) or grad_y * cst * act'(x); kind 0 SiLU, 1 shifted softplus (layers.py:21-22). */
int nq_qh_act(const float* x, const float* grad_y, int32_t kind, float cst, int64_t count, float* out, void* stream);
/* Expansion.forward (layers.py:598-662): x [R][25][Cb], weights [R][n_weights], bias [R][n_bias] (nullable) -> out [R][S][S];
 * shells_host: HOST int32[3] = number of s, p, d shells of the padded block (S = s + 3p + 5d); w3j: device [19][5][5][9] real Wigner 3j
 * tensors w3j(l1, l2, l_in)[i][j][k] in the instruction order of get_expansion_path (layers.py:664-671), zero padded. */
int nq_qh_expansion_forward(const float* x, const float* weights, const float* bias, int64_t R, int32_t Cb, const int32_t* shells_host, int32_t n_weights,
                            int32_t n_bias, const float* w3j, float* out, void* stream);
int nq_qh_expansion_backward(const float* x, const float* weights, const float* grad_out, int64_t R, int32_t Cb, const int32_t* shells_host,
                             int32_t n_weights, int32_t n_bias, const float* w3j, float* grad_x, float* grad_weights, float* grad_bias, void* stream);

/* ---- geometry bases of the Hamiltonian models --------------------------------------------------------------------------------- */
/* out [P][(order+1)^2]: real spherical harmonics Y_0..Y_order (order <= 4) of unit vectors [P][3], PhiSNet convention
 * (phisnet/nn/spherical_harmonics/spherical_harmonics.py:10-25: no 1/sqrt(4 pi), Condon-Shortley, m = -l..l). */
int nq_sph_harm(const float* unit_vectors, int64_t P, int32_t order, float* out, void* stream);
/* Adjoint of nq_sph_harm w.r.t. the vectors: gu[P][3] = sum_c grad_out[P][c] dY_c/d(x,y,z), the closed forms differentiated as polynomials of a free vector
 * (what autograd does with phisnet/nn/spherical_harmonics/spherical_harmonics_any_order.py before the chain rule through u = r/|r|): the angular half of
 * PhiSNet's forces = -dE/dR (phisnet/nn/neural_network.py:737, :981-984). */
int nq_sph_harm_backward(const float* unit_vectors, const float* grad_out, int64_t P, int32_t order, float* gu, void* stream);
/* out [P][K] = cutoff_function(r) * exp(logc_k + n_k x + v_k log(1 - e^x)), x = -alpha r  (ExponentialBernsteinRadialBasisFunctions.forward,
 * phisnet/nn/modules/exponential_bernstein_radial_basis_functions.py:36-41 == qhnet/layers.py:115-120); alpha = softplus(_alpha). */
int nq_bernstein_rbf(const float* r, int64_t P, int32_t K, float alpha, float cutoff, const float* logc, const float* n, const float* v, float* out,
                     void* stream);
int nq_bernstein_rbf_grad_alpha(const float* r, const float* grad_out, int64_t P, int32_t K, float alpha, float cutoff, const float* logc, const float* n,
                                const float* v, float* galpha_rows, void* stream);

/* gr[p] = sum_k grad_out[p][k] d rbf[p][k] / d r (cutoff function included): the radial half of PhiSNet's forces; alpha from a device scalar. */
int nq_bernstein_rbf_grad_r_dev(const float* r, const float* grad_out, int64_t P, int32_t K, const float* alpha_dev, float cutoff, const float* logc,
                                const float* n, const float* v, float* gr, void* stream);

/* The same two calls with alpha = softplus(_alpha) read from a DEVICE scalar: no host read of the learnable parameter, so a whole training step can be
 * captured into a HIP graph (trainer.GraphedStep). */
int nq_bernstein_rbf_dev(const float* r, int64_t P, int32_t K, const float* alpha_dev, float cutoff, const float* logc, const float* n, const float* v, float* out,
                         void* stream);
int nq_bernstein_rbf_grad_alpha_dev(const float* r, const float* grad_out, int64_t P, int32_t K, const float* alpha_dev, float cutoff, const float* logc,
                                    const float* n, const float* v, float* galpha_rows, void* stream);

/* The other radial bases of PhiSNet (neural_network.py:210-221), all times cutoff_function(r): kind 1 gaussian (t0 = centres, width), 2 exp-gaussian
 * (t0 = centres, width, alpha), 3 overlap-bernstein (t0 = logc, t1 = n, t2 = v, alpha), 4 bernstein (t0 = logc, t1 = n, t2 = v).  out [P][K];
 * nq_radial_basis_grad_alpha (kinds 2, 3): per-row dL/dalpha given grad_out [P][K]. */
int nq_radial_basis(int32_t kind, const float* r, int64_t P, int32_t K, float alpha, float cutoff, float width, const float* t0, const float* t1, const float* t2,
                    float* out, void* stream);
int nq_radial_basis_grad_alpha(int32_t kind, const float* r, const float* grad_out, int64_t P, int32_t K, float alpha, float cutoff, float width, const float* t0,
                               const float* t1, const float* t2, float* galpha_rows, void* stream);

/* Learnable feature-wise activations of PhiSNet on [rows][F]: kind 0 = Swish (swish.py:23-24), kind 1 = ShiftedSoftplus
 * (shifted_softplus.py:26-32).  Backward writes grad_x and per-element partials of dL/dalpha, dL/dbeta ([rows][F], sum over rows). */
int nq_feature_act(const float* x, const float* alpha, const float* beta, int64_t rows, int32_t F, int32_t kind, float* y, void* stream);
int nq_feature_act_backward(const float* x, const float* alpha, const float* beta, const float* grad_y, int64_t rows, int32_t F, int32_t kind,
                            float* grad_x, float* grad_alpha_rows, float* grad_beta_rows, void* stream);

/* The same activation on the scalar component of a packed irreps tensor [rows][ncomp][F] (PhiSNet activates xs[0] only, residual_block.py:58-64);
 * the other components are copied.  Backward partials of alpha / beta are [rows][F]. */
int nq_packed_act0(const float* x, const float* alpha, const float* beta, int64_t rows, int32_t ncomp, int32_t F, int32_t kind, float* y, void* stream);
int nq_packed_act0_backward(const float* x, const float* alpha, const float* beta, const float* grad_y, int64_t rows, int32_t ncomp, int32_t F, int32_t kind,
                            float* grad_x, float* grad_alpha_rows, float* grad_beta_rows, void* stream);

/* PhiSNet SphericalLinear (phisnet/nn/modules/spherical_linear.py:50-59; also EquiformerV2's SO3_LinearV2,
 * equiformer_v2/so3.py:587-625, order <= 6) on packed irreps tensors x, y: [rows][(order+1)^2][F]: one Linear per order,
 * y_L = x_L W_L^T (+ bias0 on the scalars), W: HOST array of order+1 device pointers to [Fout][Fin] matrices.  Forward and input gradient are one launch
 * for all orders; the weight gradient is one split-K contraction per order (scratch: nq_sph_weight_grad_scratch_floats floats; fixed summation order). */
int nq_sph_linear_forward(const float* x, const float* const* W_host, const float* bias0, float* y, int64_t rows, int32_t order, int32_t Fin, int32_t Fout,
                          void* stream);
int nq_sph_linear_input_grad(const float* grad_y, const float* const* W_host, float* grad_x, int64_t rows, int32_t order, int32_t Fin, int32_t Fout,
                             void* stream);
size_t nq_sph_weight_grad_scratch_floats(int64_t rows, int32_t order, int32_t Fin, int32_t Fout);
int nq_sph_linear_weight_grad(const float* grad_y, const float* x, float* const* grad_W_host, float* grad_bias0, int64_t rows, int32_t order, int32_t Fin,
                              int32_t Fout, float* scratch, void* stream);

/* Pair <-> atom data movement of the interaction blocks (interaction_block.py:135-142).  Rows of C floats.
 * nq_gather_rows: out[p] = x[idx[p]].  nq_segment_sum: out[n] = base[n] (nullable) + sum_{q in [seg_ptr[n], seg_ptr[n+1])} rows[order ? order[q] : q]
 * -- fixed summation order, no atomics (the reference's index_add on a GPU is not reproducible). */
int nq_gather_rows(const float* x, const int64_t* idx, int64_t P, int32_t C, float* out, void* stream);
int nq_segment_sum(const float* rows, const int64_t* order, const int64_t* seg_ptr, const float* base, int64_t N, int32_t C, float* out, void* stream);

/* ---- GemNet-OC (reference nablaDFT/gemnet_oc/) ------------------------------------------------------------------ */
/* One edge set stored as a CSR by target atom (sources ascending): ptr [atoms+1], src / dst [n], geom [n][4] = {unit vector source -> target, distance}. */
typedef struct nq_gn_set {
  int32_t n, reserved;
  const int32_t* ptr;
  const int32_t* src;
  const int32_t* dst;
  const float* geom;
} nq_gn_set;
/* All graphs of gemnet_oc.py:892-958 (get_graphs_and_indices) derived from the a2a graph (nq_graph_count / nq_graph_fill with cutoff_aint, CSR arrays
 * row_ptr / col / rev / dst; geom [E][4] is REWRITTEN with the reference's CPU arithmetic: d = torch.norm(pos[j] - pos[i]), unit vector = difference / d):
 * sub-graph selection by cutoff and the K nearest per target (utils.py:408-500, enforce_max_strictly), the symmetrised main
 * graph (gemnet_oc.py:694-775: source < target kept, flips added) with the counter-edge slot m_rev (= id_swap), the a2ee2a and qint graphs; triplet and
 * quadruplet lists (interaction_indices.py) are not materialised.  The caller owns every array: [N] counters, [N+1] prefix arrays, [E] flags / mpos / apos /
 * a_of_rev, and -- sized from the four totals nq_gn_graph_count returns -- the per-graph arrays. */
typedef struct nq_gn_graphs {
  int32_t N, E, k_main, k_aea, k_qint, reserved;
  double cutoff_main, cutoff_aea, cutoff_qint;
  const int32_t* row_ptr;
  const int32_t* col;
  const int32_t* rev;
  const int32_t* dst;
  const float* pos;
  float* geom;
  uint8_t* flags;
  int32_t *degm, *lowm, *cnt_a, *cnt_q, *tin_atom;
  int32_t *ptr_m, *lowptr_m, *ptr_a, *ptr_q, *tin_aptr;
  int32_t *m_src, *m_dst, *m_rev, *m_slot;
  float* m_geom;
  int32_t *a_src, *a_dst;
  float* a_geom;
  int32_t* a_of_rev;
  int32_t *q_src, *q_dst;
  float* q_geom;
  int32_t* tin_ptr;
  int32_t *mpos, *apos;
  int32_t *tin_main, *q_of_rev, *qpos;
} nq_gn_graphs;
/* totals_host[4] = {main edges, a2ee2a edges, qint edges, rows of the (qint edge, main in-edge of its source) table}; synchronises `stream`.
 * max_degree: largest a2a in-degree (<= 512). */
int nq_gn_graph_count(const void* graphs /* nq_gn_graphs* */, int32_t max_degree, int32_t* totals_host, void* stream);
int nq_gn_graph_fill(const void* graphs /* nq_gn_graphs* */, void* stream);
/* RadialBasis (layers/radial_basis.py:196-220): out[n][R] = scale * envelope_p(d/cutoff) * exp(coeff (d/cutoff - offset_k)^2); d = geom[.][3]. */
int nq_gn_radial_basis(const float* geom, int64_t n, int32_t num_radial, const float* offset, double cutoff, double exponent, float scale, float* out,
                       void* stream);
/* EfficientInteractionBilinear's first contraction (layers/efficient.py:213-229) for the triplet families (interaction_indices.py:13-118):
 * S[o][s][c] = sum over in-edges p of target(o) in `in_set` with source(p) != source(o) of Y_s0(clamp(v_o . v_p)) * scale * x[p][c];  backward: d x. */
int nq_gn_triplet_forward(const void* out_set, const void* in_set, const float* x, int32_t C, int32_t NS, float scale, float* S, void* stream);
int nq_gn_triplet_backward(const void* out_set, const void* in_set, const float* dS, int32_t C, int32_t NS, float scale, float* dx, void* stream);
/* Quadruplets (interaction_indices.py:121-282, angles gemnet_oc.py:597-655, "legendre_outer" basis spherical_basis.py:104-110): x rows are indexed
 * tin_ptr[q] + j (j-th main in-edge of source(q)); S[o][l * NS + l'][c].  backward scratch: f32[main edges * KQ * NS * C], KQ >= largest qint in-degree. */
int nq_gn_quad_forward(const void* main_set, const void* qint_set, const int32_t* tin_ptr, int32_t n_atoms, const float* x, int32_t C, int32_t NS, float scale,
                       float* S, void* stream);
int nq_gn_quad_backward(const void* main_set, const void* qint_set, const int32_t* tin_ptr, int32_t n_atoms, int64_t T, const float* dS, int32_t C, int32_t NS,
                        int32_t KQ, float scale, float* scratch, float* dx, void* stream);
/* Tuning hook (process-global): 1 = one workgroup per centre atom with LDS-shared bases (default), 0 = one thread per (edge, channel). */
void nq_gn_set_quad_variant(int32_t variant);
/* BasisEmbedding without inner index (layers/efficient.py:136-141): cir[(q, j)][i] = sum_s rad_w1[q][i * NS + s] Y_s0(v_q . v_p) * scale. */
int nq_gn_cir_forward(const void* main_set, const void* qint_set, const int32_t* tin_ptr, int64_t T, const float* rad_w1, int32_t I, int32_t NS, float scale,
                      float* cir, void* stream);
int nq_gn_cir_backward(const void* main_set, const void* qint_set, const int32_t* tin_ptr, const float* dcir, int32_t I, int32_t NS, float scale,
                       float* d_rad_w1, void* stream);
/* rad_W1 @ sph_m (layers/efficient.py:231-244): out[o][i][c] = sum_s R[o][i * NSS + s] S[o][s][c]; backward writes dR and / or dS (nullable). */
int nq_gn_rowmm_forward(const float* R, const float* S, int64_t n, int32_t I, int32_t NSS, int32_t C, float* out, void* stream);
int nq_gn_rowmm_backward(const float* R, const float* S, const float* dout, int64_t n, int32_t I, int32_t NSS, int32_t C, float* dR, float* dS, void* stream);
/* PairInteraction (layers/interaction_block.py:721-733): out[a][r][c] = sum_{p in row(a)} rad_w[p][r] x[source(p)][c]; the a2a graph is symmetric (rev). */
int nq_gn_pair_forward(const void* a2a_set, const float* rad_w, const float* x, int32_t N, int32_t Rr, int32_t C, float* out, void* stream);
int nq_gn_pair_backward(const void* a2a_set, const int32_t* rev, const float* rad_w, const float* x, const float* dout, int32_t N, int32_t Rr, int32_t C,
                        float* d_rad_w, float* dx, void* stream);
/* Adjoint of the row gather x_tin[row] = x[tin_main[row]] of the quadruplet path (interaction_block.py:579: x_db[idx["triplet_in"]["in"]]):
 * out[p] = sum over the qint edges q whose source is target(p) of g[tin_ptr[q] + position of p in its row]; a2a_row_ptr / q_of_rev from nq_gn_graphs. */
int nq_gn_tin_scatter(const void* main_set, const int32_t* a2a_row_ptr, const int32_t* q_of_rev, const int32_t* tin_ptr, const float* g, int32_t C,
                      float* out, void* stream);
/* EdgeEmbedding input (layers/embedding_block.py:85-90): cat[e] = [h[source] | h[target] | m[e]]; backward_h: dh from the first two blocks of dcat. */
int nq_gn_cat_forward(const void* main_set, const float* h, const float* m, int32_t A, int32_t Em, float* cat, void* stream);
int nq_gn_cat_backward_h(const void* main_set, const int32_t* rev, const float* dcat, int32_t N, int32_t A, int32_t Em, float* dh, void* stream);
/* AtomUpdateBlock / OutputBlock head (layers/atom_update_block.py:88-93): out[a][c] = sum_{p in row(a)} m[p][c] r[p][c]. */
int nq_gn_mulsum_forward(const void* main_set, const float* m, const float* r, int32_t N, int32_t C, float* out, void* stream);
int nq_gn_mulsum_backward(const void* main_set, const float* m, const float* r, const float* dout, int32_t C, float* dm, float* dr, void* stream);
/* Direct forces (gemnet_oc.py:1216-1243): per-edge scalar, averaged with the counter-edge if coupled, times the edge vector, summed per target atom. */
int nq_gn_forces_forward(const void* main_set, const int32_t* rev, const float* f_edge, int32_t N, int32_t coupled, float* forces, void* stream);
int nq_gn_forces_backward(const void* main_set, const int32_t* rev, const float* d_forces, int32_t coupled, float* d_f_edge, void* stream);
/* out[p] = x[idx[p]] (* y[p] if y); out[n] = sum_{q in [ptr[n], ptr[n+1])} rows[r] (* y[r] if y), r = order ? order[q] : q, entries r < 0 skipped;
 * out = a * b;  out = alpha a + beta b (b nullable);  dW[t] = sum_{n: z[n] == t + 1} g[n] (Embedding(z - 1), layers/embedding_block.py:39-53). */
int nq_gn_gather(const float* x, const int32_t* idx, const float* y, int64_t P, int32_t C, float* out, void* stream);
int nq_gn_segment_sum(const float* rows, const float* y, const int32_t* order, const int32_t* ptr, int64_t N, int32_t C, float* out, void* stream);
int nq_gn_mul(const float* a, const float* b, int64_t n, float* out, void* stream);
int nq_gn_lincomb(const float* a, const float* b, float alpha, float beta, int64_t n, float* out, void* stream);
/* out = scale * g * d/dz [silu(z) / 0.6] (adjoint of ScaledSiLU with a folded constant). */
int nq_gn_ssilu_backward(const float* z, const float* g, float scale, int64_t n, float* out, void* stream);
int nq_gn_embed_grad(const int32_t* z, const float* g, int32_t N, int32_t num_elements, int32_t C, float* dW, void* stream);

/* ---- eSCN building blocks (reference nablaDFT/escn/escn.py, so3.py) --------------------------------------------------- */
/* Directed radius graph of escn.py:253-255 (radius_graph(pos, r, batch, max_num_neighbors)): per target atom the first K atoms of its molecule (index
 * order) with d^2 < r^2.  Pass 1 (count): deg [N], ptr [N+1], *E_host (synchronises).  Pass 2 (fill): src, dst [E], geom [E][4] = {pos[j] - pos[i], |.|}. */
int nq_es_graph_count(const float* pos, const int32_t* mol_ptr, const int32_t* atom_mol, int32_t N, double cutoff, int32_t K, int32_t* deg, int32_t* ptr,
                      int32_t* E_host, void* stream);
int nq_es_graph_fill(const float* pos, const int32_t* mol_ptr, const int32_t* atom_mol, int32_t N, double cutoff, int32_t K, const int32_t* ptr, int32_t* src,
                     int32_t* dst, float* geom, void* stream);
/* Edge rotation matrices rot [E][3][3] (escn.py:435-487; deterministic helper axis instead of the reference's random vector: same model output). */
int nq_es_frames(const float* geom, int32_t E, float* rot, void* stream);
/* Wigner-D rows (so3.py:377-425): W [E][n_red][n_full], row b = row red_row[b] of the degree-red_l[b] block D^l = Z(alpha) J_l Z(beta) J_l Z(gamma);
 * J: the J_l matrices back to back (J_offset[l]); scratch: 8-byte aligned, 3 E doubles (the Euler angles and all trigonometry are evaluated in float64:
 * the rows are then exact to float32 rounding, the reference's float32 evaluation carries several 1e-6 near the polar axis). */
int nq_es_wigner(const float* rot, int32_t E, const float* J, const int32_t* J_offset, const int32_t* red_l, const int32_t* red_row, int32_t n_red, int32_t n_full,
                 int32_t lmax, float* scratch, float* W, void* stream);
/* GaussianSmearing (smearing.py:14-31): out[e][k] = exp(coeff (geom[e][3] - offset[k])^2). */
int nq_es_smearing(const float* geom, int64_t E, int32_t K, const float* offset, float coeff, float* out, void* stream);
/* One small matrix per row times the row's [coefficients][channels] block (SO3_Embedding._rotate / _rotate_inv / to_grid / from_grid, so3.py:265-375):
 * transpose == 0: out[o][i][c] (+)= sum_s R_o[i][s] X_r[s][c];  else out[o][s][c] (+)= sum_i R_o[i][s] X_r[i][c];  R_o = R + o * r_stride (0: shared),
 * r = index ? index[o] : o; strides in floats; R is I x NSS. */
int nq_rowop(const float* R, int64_t r_stride, const float* X, int64_t x_stride, const int32_t* index, float* out, int64_t out_stride, int64_t n, int32_t I,
             int32_t NSS, int32_t C, int32_t transpose, int32_t accumulate, void* stream);

/* nq_rowop with one side living in per-block tensors (the m-blocks an SO(2) layer consumes / produces): seg_side 0 = the I side (rows of R), 1 = the S side
 * (columns); seg_rows[nseg] (host) rows per block, seg_ptrs[nseg] (host array of device pointers) the contiguous [n][rows_k][C] tensors; x_or_out / stride: the
 * other side (transpose == 0: S side in, I side out; else I side in, S side out).  nseg <= 8. */
int nq_rowop_blocks(const float* R, int64_t r_stride, float* x_or_out, int64_t stride, const int32_t* index, int32_t seg_side, int32_t nseg,
                    const int32_t* seg_rows, float* const* seg_ptrs, int64_t n, int32_t I, int32_t NSS, int32_t C, int32_t transpose, int32_t accumulate,
                    void* stream);
/* Fused S2 activation of the SO(2) message blocks (escn/so3.py:301-318 to_grid / from_grid around the point-wise SiLU; equiformer_v2/activation.py:155-176):
 * y_blocks = from_grid(SiLU(to_grid(x_blocks))) in ONE kernel on the matrix cores, the [n][G][C] grid tensor never reaches memory; backward != 0: dx_blocks from
 * (x_blocks, dy_blocks) with the grid recomputed.  T, F: [G][S] to_grid / from_grid matrices; blocks: nseg contiguous tensors [n][seg_rows[k]][C] (HOST arrays of
 * device pointers), S = sum seg_rows.  Requires C % 64 == 0, S <= 32, G <= 96 (NQ_ERR_ARG otherwise). */
int nq_s2_activation_blocks(const float* T, const float* F, int32_t G, int32_t S, int32_t C, int64_t n, int32_t nseg, const int32_t* seg_rows, float* const* x_ptrs,
                            float* const* gy_ptrs, float* const* out_ptrs, int32_t backward, void* stream);

/* Rotations that use the degree-block structure of the Wigner rows (235 of 29 x 49 entries at lmax 6 / mmax 2), no LDS.  nq_es_rotate (SO3_Embedding._rotate):
 * block(i)[o][row][c_off + c] = sum_k W_o[i][l_i^2 + k] x[index ? index[o] : o][l_i^2 + k][c]; red_l [n_red] (HOST) = degree of every kept row, rows in W's
 * order; blocks = nseg contiguous tensors [E][seg_rows_k][c_stride] (HOST arrays; two rotations may fill two channel halves of one block).
 * nq_es_rotate_back (_rotate_inv fused with _reduce_edge): out[n][s][c] = coef_scale[s] sum_{q in [ptr[n], ptr[n+1])} sum_i W_o[i][s] block(i)[o][row][c_off + c],
 * o = order ? order[q] : q; ptr == NULL: one output row per edge; coef_scale nullable. */
int nq_es_rotate(const float* W, int64_t w_stride, const float* x, int64_t x_stride, const int32_t* index, int32_t nseg, const int32_t* seg_rows,
                 float* const* seg_ptrs, int32_t c_stride, int32_t c_off, int64_t E, const int32_t* red_l, int32_t n_red, int32_t lmax, int32_t C, void* stream);
int nq_es_rotate_back(const float* W, int64_t w_stride, int32_t nseg, const int32_t* seg_rows, float* const* seg_ptrs, int32_t c_stride, int32_t c_off,
                      const int32_t* ptr, const int32_t* order, const float* coef_scale, float* out, int64_t n_out, const int32_t* red_l, int32_t n_red,
                      int32_t lmax, int32_t C, void* stream);

/* ---- EquiformerV2 building blocks (reference nablaDFT/equiformer_v2/; the graph, rotations, S2 grids and SO(2) GEMMs are the eSCN entries
 * above, SO3_LinearV2 is nq_sph_linear_*) ------------------------------------------------------------------------------------------------------------------ */
/* torch.nn.LayerNorm over rows of width W (radial_function.py:20, transformer_block.py:151): rows may be strided (x_stride / y_stride floats); stats [rows][2]
 * (mean, rstd) out.  Backward: grad_x, grad_weight [W], grad_bias [W] (fixed summation order); scratch nq_eq_layernorm_scratch_floats floats. */
int nq_eq_layernorm_forward(const float* x, int64_t x_stride, const float* weight, const float* bias, int64_t rows, int32_t W, float eps, float* y, int64_t y_stride,
                            float* stats, void* stream);
size_t nq_eq_layernorm_scratch_floats(int64_t rows, int32_t W);
int nq_eq_layernorm_backward(const float* x, int64_t x_stride, const float* weight, const float* grad_y, int64_t g_stride, const float* stats, int64_t rows, int32_t W,
                             float* grad_x, int64_t gx_stride, float* grad_weight, float* grad_bias, float* scratch, void* stream);
/* EquivariantLayerNormArraySphericalHarmonics (layer_norm.py:117-215, normalization "component", std_balance_degrees): x, y [N][(lmax+1)^2][C]; LayerNorm
 * (w0, b0) on the scalars; all l > 0 scaled by (mean_c sum_i balance_weight[i] x_ic^2 + eps)^-1/2 affine_weight[l-1][c]; stats [N][3] out; 1 <= lmax <= 6. */
int nq_eq_norm_sh_forward(const float* x, const float* w0, const float* b0, const float* affine_weight, const float* balance_weight, int64_t N, int32_t lmax,
                          int32_t C, float eps, float* y, float* stats, void* stream);
size_t nq_eq_norm_sh_scratch_floats(int64_t N, int32_t lmax, int32_t C);
int nq_eq_norm_sh_backward(const float* x, const float* w0, const float* affine_weight, const float* balance_weight, const float* grad_y, const float* stats,
                           int64_t N, int32_t lmax, int32_t C, float* grad_x, float* grad_w0, float* grad_b0, float* grad_affine_weight, float* scratch,
                           void* stream);
/* Attention logits (transformer_block.py:343-350; activation.py:52-61): z[e][h] = sum_a alpha_dot[h][a] SmoothLeakyReLU_0.2(x[e][h][a]). */
int nq_eq_logits_forward(const float* x, const float* alpha_dot, int64_t E, int32_t H, int32_t A, float* z, void* stream);
size_t nq_eq_logits_scratch_floats(int64_t E, int32_t H, int32_t A);
int nq_eq_logits_backward(const float* x, const float* alpha_dot, const float* grad_z, int64_t E, int32_t H, int32_t A, float* grad_x, float* grad_alpha_dot,
                          float* scratch, void* stream);
/* torch_geometric.utils.softmax(z, edge_index[1]) (transformer_block.py:352) for edges sorted by target: the in-edges of atom n are [ptr[n], ptr[n+1]). */
int nq_eq_softmax_forward(const float* z, const int32_t* ptr, int64_t N, int32_t H, float* out, void* stream);
int nq_eq_softmax_backward(const float* y, const float* grad_y, const int32_t* ptr, int64_t N, int32_t H, float* grad_z, void* stream);
/* Messages times attention weights (transformer_block.py:357-370) on the per-block tensors x_b [E][rows_b][H V] (host arrays of device pointers, nseg <= 8),
 * alpha [E][H].  grad == NULL: out_b = x_b alpha.  Else out_b = grad_b alpha and (grad_alpha != NULL) grad_alpha [E][H] = sum_b sum_rows,v grad_b x_b. */
int nq_eq_head_scale(int32_t nseg, const int32_t* rows, const float* const* x, const float* const* grad, const float* alpha, int64_t E, int32_t H, int32_t V,
                     float* const* out, float* grad_alpha, void* stream);
/* out[n][i][c] = x[n][i][c] * row_scale[row_index ? row_index[n] : n] * coef_scale[i] (nullable factors): the rescale of SO3_Rotation.rotate_inv
 * (so3.py:121-136,338-343) and GraphDropPath (drop.py:57-71). */
int nq_eq_scale(const float* x, const float* row_scale, const int32_t* row_index, const float* coef_scale, int64_t N, int32_t I, int32_t C, float* out, void* stream);

/* ---- loss / optimizer ------------------------------------------------------------------------ */
/* loss[1] = coef_e * mean|E-y| + coef_f * mean_i ||F_i - Ft_i||_2 ; grad_energy[B], grad_forces[N][3] */
int nq_loss_l1_l2(const float* energy, const float* y, int32_t B, const float* forces, const float* f_target, int32_t N, float coef_e,
                  float coef_f, float* loss, float* grad_energy, float* grad_forces, void* stream);
/* loss[1] = coef_e * mean (E-y)^2 + coef_f * mean_{i,c} (F_ic - Ft_ic)^2  -- torch.nn.MSELoss on both outputs, the loss of the
 * schnetpack task (config/model/painn.yaml:30-46, weights loss_weight) */
int nq_loss_mse(const float* energy, const float* y, int32_t B, const float* forces, const float* f_target, int32_t N, float coef_e,
                float coef_f, float* loss, float* grad_energy, float* grad_forces, void* stream);
/* clip_grad_norm_(max_norm) (skipped if max_norm <= 0) + AdamW step over the flat buffers; step >= 1;
 * scratch: f32[512]. */
int nq_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t count, float max_norm, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int32_t step, float* scratch, void* stream);

/* ---- measurement hook ------------------------------------------------------------------------- */
/* Opt-in per-kernel timing with HIP events recorded on the launch stream (bench.py roofline leg).
 * Process-global and not thread-safe: enable it only around a single-threaded measurement.
 * nq_profile_read synchronises the device, writes up to `cap` rows {name (name_stride bytes, NUL
 * terminated), total milliseconds, launch count}, clears the records and returns the number of names. */
void nq_profile_enable(int32_t on);
int nq_profile_read(char* names_host, int32_t name_stride, double* total_ms_host, int64_t* counts_host, int32_t cap);
/* As nq_profile_read, plus flops_host[i] (nullable) = arithmetic of the launches of name i: the dense-product launchers record 2 M N K per call, so a
 * class's TFLOP/s is flops / time without re-deriving shapes from names (every other launcher records 0).  ABI 11. */
int nq_profile_read2(char* names_host, int32_t name_stride, double* total_ms_host, int64_t* counts_host, double* flops_host, int32_t cap);

/* Engine / tuning switch of the dense products (process-global; default 1; the bits are named by enum GemmVariant in csrc/gemm.hip):
 *   bits 0-1  generic round-1 kernel flavour (bit0 = 8 wavefronts per 128x128 tile, bit1 = register prefetch),
 *   bit 3 (8)   never the small-problem kernel,  bit 4 (16)  only the generic kernels (no k_gemm2 / k_gemm3),
 *   bit 5 (32)  exact-f32 MFMA only: every product on v_mfma_f32_32x32x2_f32.  Without it (the default) launches of >= 192 tiles of 128x128 run on the
 *               split-bf16 engine (csrc/gemm_split.h): each f32 operand value is split EXACTLY into three bf16 pieces and a product is the sum of six
 *               piece products on v_mfma_f32_32x32x16_bf16 with f32 accumulation -- f32-accurate (error vs float64 measured <= the exact engine's),
 *               1.3-1.7x faster, but a row's bits then depend on which engine the launch size selects, and non-finite operands give NaN where the
 *               exact engine would give inf.  The environment variable NQ_GEMM_F32=1 (read once) has the same effect as bit 5.
 *   bit 6 (64)  the split-bf16 engine for EVERY launch it can run, whatever the size (tests: the golden vectors with all products on it).
 *   bit 8 (256) spherical linears on the row-mapped generic kernel (default since round 4: one plain strided product per packed component as ONE batched
 *               launch of the tile engines, grid.y = component).
 *   bit 7 (128) never split the contraction of a forward / input-gradient product (default: contractions of >= 2048 with fewer than 256 output tiles of
 *               128x128 are cut into up to 16 ranges, partial slabs in a library-owned per-stream scratch, fixed-order reduction; round 4).
 * The weight-gradient scratch size does not depend on the switch. */
void nq_set_gemm_variant(int32_t variant);
/* The split-K scratch (bit 7 above) is one grow-only device buffer per (device, stream), owned by the library.  A buffer that was handed out while its stream
 * was capturing is never freed or moved afterwards (the captured graph replays into the raw pointer): when a later eager call needs more, the old buffer is
 * retired and a new one allocated; inside a capture nothing is allocated (a too small buffer means the plain, unsplit launch).  nq_gemm_splitk_release frees
 * every buffer of the current device, retired ones included -- call it only when no graph that used them will be replayed again.  nq_gemm_splitk_state is the
 * test hook: current pointer, size in floats, captured flag and number of retired buffers of one stream. */
void nq_gemm_splitk_release(void);
int nq_gemm_splitk_state(void* stream, uint64_t* ptr, uint64_t* floats, int32_t* captured, int32_t* retired);

/* ---- building blocks exported for unit tests ----------------------------------------------- */
/* C[M,N] = A[M,K] W[N,K]^T (+bias[N]); if C_silu != NULL also writes silu(C). */
int nq_linear_forward(const float* A, const float* W, const float* bias, float* C, float* C_silu, int32_t M, int32_t N, int32_t K,
                      void* stream);
/* C[M,N] = A W^T and C_act = alpha * resid (nullable) + beta * silu(C): Dense + ScaledSiLU (+ residual) of gemnet_oc/layers/base_layers.py:11-97 in one pass. */
int nq_linear_forward_act(const float* A, const float* W, float* C, float* C_act, const float* resid, float alpha, float beta, int32_t M, int32_t N,
                          int32_t K, void* stream);
/* C[M,N] = alpha * aux + A[M,K] W[N,K]^T  (aux [M,N], not aliasing C): the second product of a two-term sum in the epilogue of the GEMM -- the +-m pairs of
 * the SO(2) convolutions (escn.py:858-877 `x_r[:, 0] - x_i[:, 1]`, `x_r[:, 1] + x_i[:, 0]`; equiformer_v2 so2_ops.py:53-61) without a separate pass.  ABI 13. */
int nq_linear_forward_res(const float* A, const float* W, const float* aux, float alpha, float* C, int32_t M, int32_t N, int32_t K, void* stream);
/* bf16 MFMA variants (fp32 operands in HBM rounded to bf16 on the way into LDS, fp32 accumulation; BASELINE.json configs[2] names bf16 for GemNet-OC):
 * nq_bf16_pack: W [N][K] fp32 -> Wb [N][K], WbT [K][N] (bf16, round to nearest even).  nq_linear_forward_bf16: as nq_linear_forward_act with W = Wb (C_act
 * nullable -> plain store); K % 32 == 0.  nq_linear_input_grad_bf16: C[M,K] (+)= G[M,N] W[N,K] with W given as WbT; N % 32 == 0. */
int nq_bf16_pack(const float* W, int32_t N, int32_t K, void* Wb, void* WbT, void* stream);
int nq_linear_forward_bf16(const float* A, const void* Wb, float* C, float* C_act, const float* resid, float alpha, float beta, int32_t M, int32_t N,
                           int32_t K, void* stream);
int nq_linear_input_grad_bf16(const float* G, const void* WbT, float* C, int32_t M, int32_t N, int32_t K, int32_t accumulate, void* stream);
/* gW[N][K] = G[rows][N]^T X[rows][K] on the bf16 MFMA (operands transposed into bf16 copies inside `scratch`, split over the rows, fixed-order reduction). */
size_t nq_weight_grad_bf16_scratch_bytes(int64_t rows, int32_t N, int32_t K);
int nq_linear_weight_grad_bf16(const float* G, const float* X, float* gW, int64_t rows, int32_t N, int32_t K, void* scratch, void* stream);
/* bf16-in-memory flavours of the same kernels (gemnet_oc.set_gemm_precision("bf16_act"); ScaledSiLU / ResidualLayer of layers/base_layers.py:11-97): tensors
 * that only another of these products or the SiLU reverse reads stay bf16 in HBM.  All roundings are the round-to-nearest-even conversion of the staging path,
 * so every result is bitwise the fp32-in-memory kernel's result rounded (outputs) or the fp32 kernel's result on the widened operand (inputs).
 * nq_linear_forward_bf16_out (layers/base_layers.py:11-97): as nq_linear_forward_bf16 with C_act given; A is fp32 [M][K], or bf16 [M][K] if a_bf16; the
 *   pre-activation is written as bf16 [M][N]; `act` = alpha * resid + beta * silu(pre) (from the unrounded accumulator) is written as bf16 if act_bf16, else
 *   fp32.  A and Wb 16-byte aligned; the outputs need only their natural alignment, N is arbitrary.
 * nq_linear_weight_grad_bf16_x (layers/base_layers.py:11-97): nq_linear_weight_grad_bf16 with X given as bf16 [rows][K]; same scratch.
 * nq_gn_ssilu_backward_bf16 (layers/base_layers.py:11-97): nq_gn_ssilu_backward with z given as bf16 [n]. */
int nq_linear_forward_bf16_out(const void* A, int32_t a_bf16, const void* Wb, void* pre_bf16, void* act, int32_t act_bf16, const float* resid, float alpha,
                               float beta, int32_t M, int32_t N, int32_t K, void* stream);
int nq_linear_weight_grad_bf16_x(const float* G, const void* X_bf16, float* gW, int64_t rows, int32_t N, int32_t K, void* scratch, void* stream);
int nq_gn_ssilu_backward_bf16(const void* z_bf16, const float* g, float scale, int64_t n, float* out, void* stream);
/* C[M,K] (+)= G[M,N] W[N,K] */
int nq_linear_input_grad(const float* G, const float* W, float* C, int32_t M, int32_t N, int32_t K, int32_t accumulate, void* stream);
/* Input gradient with a fused epilogue on C[M,K] = G W: mode 1: C = beta * (G W) * silu'(aux) (adjoint of the activation below), mode 2: C = alpha * aux + G W
 * (skip connection of the adjoint); aux [M,K].  _bf16_epi: the same on the bf16 MFMA kernel (W given as WbT, N % 32 == 0). */
int nq_linear_input_grad_epi(const float* G, const float* W, float* C, int32_t M, int32_t N, int32_t K, const float* aux, float alpha, float beta, int32_t mode,
                             void* stream);
int nq_linear_input_grad_bf16_epi(const float* G, const void* WbT, float* C, int32_t M, int32_t N, int32_t K, const float* aux, float alpha, float beta,
                                  int32_t mode, void* stream);
/* gW[N,K] = G[rows,N]^T X[rows,K]; scratch: f32[nq_weight_grad_scratch_floats(rows,N,K)] */
/* out[c] = sum over rows of A[r][c] (row stride lda floats) in a fixed order (per-chunk partial sums, then the chunks in order): the bias gradient of a
 * Linear layer (torch.nn.Linear backward); scratch: nq_column_sum_scratch_floats(rows, cols) floats. */
size_t nq_column_sum_scratch_floats(int64_t rows, int32_t cols);
int nq_column_sum(const float* A, int64_t rows, int32_t cols, int64_t lda, float* out, float* scratch, void* stream);
size_t nq_weight_grad_scratch_floats(int64_t rows, int32_t N, int32_t K);
int nq_linear_weight_grad(const float* G, const float* X, float* gW, int64_t rows, int32_t N, int32_t K, float* scratch, void* stream);
/* The same launch also produces the bias gradient gb[N] = column sums of G (taken from the operand registers on their way into LDS: no separate pass over G;
 * torch.nn.Linear backward); same scratch size. */
int nq_linear_weight_grad_bias(const float* G, const float* X, float* gW, float* gb, int64_t rows, int32_t N, int32_t K, float* scratch, void* stream);

/* ---- Data-parallel gradient exchange over RCCL (round 4; SURVEY 8(b) `nq_allreduce`) -------------------------------------------------------
 * Replaces: Lightning DDPStrategy's gradient all-reduce (nablaDFT/utils/pipelines.py:65-68, `strategy: ddp` of the config yaml files).  One process
 * per GPU; the only thing ever exchanged is the flat fp32 gradient buffer (one conformer = one graph: no data-path collective).  librccl.so is bound with
 * dlopen at the first call (no link-time dependency; nq_rccl_available() = 0 and NQ_ERR_ARG from the other entry points if it cannot be loaded).
 * Job set-up: rank 0 calls nq_rccl_unique_id (128 bytes) and hands the bytes to every rank through any side channel (nabladft_amd/dist.py uses the
 * torch.distributed store); every rank calls nq_rccl_comm_create with its HIP device current.  The collectives are enqueued on `stream` (ordered after the
 * kernels that wrote `buf`, before the optimiser kernel; no host synchronisation).  nq_allreduce: buf <- sum over ranks (in place, fp32);
 * nq_allreduce_mean: sum, then * 1/world on the same stream; nq_rccl_broadcast: buf of `root` -> all (initial parameters). */
int nq_rccl_available(void);
int nq_rccl_unique_id(void* id128);
int nq_rccl_comm_create(const void* id128, int32_t world, int32_t rank, void** comm);
int nq_rccl_comm_destroy(void* comm);
int nq_rccl_comm_count(void* comm, int32_t* count);   /* ncclCommCount: the ranks RCCL itself sees (bench.py reports it as config.collective.ranks_seen) */
int nq_allreduce(float* buf, size_t n, void* comm, void* stream);
int nq_allreduce_mean(float* buf, size_t n, void* comm, void* stream);
int nq_rccl_broadcast(float* buf, size_t n, int32_t root, void* comm, void* stream);

/* ---- Batched L-BFGS geometry optimisation, state on the device (ABI 17; csrc/lbfgs.hip) -----------------------------------------------------
 * Replaces: ASEBatchwiseLBFGS.step / update / determine_step (nablaDFT/optimization/optimizers.py:437-605, the branch without line search), the
 * fixed-atom zeroing of BatchwiseCalculator.get_forces (optimization/calculator.py:85-86), the per-step positions -> float32 model input of
 * atoms_list_to_PYG (optimization/opt_utils.py) and the convergence test of BatchwiseOptimizer.converged (optimizers.py:244-249).  All arithmetic is float64.
 * `state` is ONE caller-owned device buffer of nq_lbfgs_state_bytes(N, B, memory) bytes, 16-byte aligned (0 = bad dimensions, see nq_last_error).
 * nq_lbfgs_state_layout fills offsets_host[10] with the byte offsets of: header int32[16] = {iteration, unconverged molecules at the last step (-2: the
 * step was called with other N / B / memory / n_small than nq_lbfgs_init and did nothing), first iteration at which no molecule was unconverged (-1: none
 * yet), normalisations so far, N, B, memory, n_small, 2 internal words}; mol_ptr int32[B+1]; order int32[B]; converged int32[B]; rho f64[memory][B];
 * r f64[N][3] (master positions); r0; f0; S f64[memory][N][3]; Y f64[memory][N][3] (pair k of a run sits in ring slot k % memory).
 * nq_lbfgs_init: mol_ptr_host is a HOST array [B+1]; every molecule needs 1..512 atoms (NQ_ERR_MOL_TOO_LARGE above), memory 1..1024; copies `pos`
 * (float32, or float64 when pos_f64) into r and into pos32 (the model's input tensor), zeroes the counters, writes *n_small_host (molecules of <= 192 atoms,
 * one wavefront each; the others take one workgroup each) and synchronises `stream` once.
 * nq_lbfgs_step: ONE kernel launch = one optimiser step on the forces of the current positions (float32, or float64 when forces_f64; fixed_mask uint8[N]
 * nullable, non-zero = atom fixed): history push, two-loop recursion with H0 = 1/alpha, per-molecule maxstep scaling, damping, r += dr, pos32 = (float) r,
 * r0 / f0, converged flags, header.  Molecules with max_i |f_i|^2 < fmax^2 do not move.  evaluate_only != 0: only the converged flags, the unconverged
 * count and the latch are written (the final convergence test of BatchwiseDynamics.irun, optimizers.py:108-111); the iteration does not advance.
 * Results are bitwise reproducible and do not depend on which other molecules share the batch. */
size_t nq_lbfgs_state_bytes(int32_t N, int32_t B, int32_t memory);
int nq_lbfgs_state_layout(int32_t N, int32_t B, int32_t memory, size_t* offsets_host);
int nq_lbfgs_init(void* state, size_t state_bytes, const int32_t* mol_ptr_host, int32_t N, int32_t B, int32_t memory, const void* pos, int32_t pos_f64,
                  float* pos32, int32_t* n_small_host, void* stream);
/* nq_lbfgs_step repeats N, B, memory and n_small (the launch geometry is computed from them on the host, without reading the device).  The kernel compares
 * them with the header nq_lbfgs_init wrote; on a mismatch it touches nothing but header word 1, which it sets to -2: the call still returns NQ_OK (it was
 * enqueued), and the caller sees the -2 at its next read of the header. */
int nq_lbfgs_step(void* state, int32_t N, int32_t B, int32_t memory, int32_t n_small, const void* forces, int32_t forces_f64, const uint8_t* fixed_mask,
                  float* pos32, double fmax, double maxstep, double damping, double alpha, int32_t evaluate_only, void* stream);

/* ---- Batched molecular dynamics, state on the device (csrc/md.hip; entry points added, ABI 17 unchanged) ------------------------------------------------------------------------
 * Replaces: PYGAseInterface.init_md / run_md (nablaDFT/optimization/pyg_ase_interface.py:207-263, 284-294: ase VelocityVerlet :239, ase Langevin :241-246),
 * _init_velocities (:265-282: MaxwellBoltzmannDistribution, Stationary, ZeroRotation), the FixAtoms constraint (:159-162) and the MDLogger / Trajectory
 * observers (:251-263) as device rings.  ase is not in the reference tree: the equations are restated (nabladft_amd/md.py) and unpinned against ase.
 * Units: Hartree, Angstrom, amu, fs, K.  nq_md_constants writes {KAPPA, KB}: (Hartree/Angstrom)/amu -> Angstrom/fs^2 and Hartree/K from CODATA 2014.
 * All state is float64.  flags: 1 = log ring, 2 = frame ring, 4 = frames carry velocities too; a requested ring with capacity 0 is NQ_ERR_ARG.
 * `state` is ONE caller-owned device buffer of nq_md_state_bytes(...) bytes, 16-byte aligned (0 = bad dimensions, see nq_last_error).  nq_md_state_layout
 * fills offsets_host[12] with the byte offsets of: header int32[32] = {steps taken, status (-2: a call came with other dimensions than nq_md_init and did
 * nothing), pending (a first half-step waits for its second half-kick), log rows in the ring, frames in the ring, overflow flag (a sample found its ring full
 * and was dropped), N, B, n_small, log capacity, frame capacity, flags, last sampled step, internal}; mol_ptr int32[B+1]; order int32[B]; mol_key int64[B];
 * mass f64[N]; fixed uint8[N]; r f64[N][3]; v f64[N][3]; rv f64[N][3] (rnd_vel of a pending step with injected noise); log f64[cap][B][8] = {step, E_tot,
 * E_pot, E_kin (Hartree), T (K, dof = 3 (n - n_fixed)), |P| (amu Angstrom/fs), |L| about the centre of mass (amu Angstrom^2/fs), 0}; frames f64[cap][N][3];
 * velocity frames f64[cap][N][3].  The host drains a ring by copying its rows and writing 0 to header word 3 / 4 on the same stream.
 * nq_md_init: mol_ptr_host, mol_key_host (nullable: the molecule's index), masses_host (amu, every one > 0 or NQ_ERR_ARG) and fixed_host (nullable uint8[N])
 * are HOST arrays; every molecule needs 1..512 atoms (NQ_ERR_MOL_TOO_LARGE above); copies `pos` (float32, or float64 when pos_f64) into r and pos32 (the
 * model's input tensor) and `vel` (device f64[N][3], nullable: zero) into v, writes *n_small_host, synchronises `stream` once.
 * nq_md_init_velocities: v = zeta sqrt(KAPPA KB T_init / m), then (flags) v -= sum(m v) / sum(m) and v -= omega x (x - x_com) with I omega = L solved in the
 * eigenbasis of the inertia tensor (eigenvalues <= 1e-10 trace(I) are skipped: atoms, diatomics, linear molecules); fixed atoms keep v = 0.
 * nq_md_step: ONE kernel launch = one MD step, given the forces (float32, or float64 when forces_f64) and optionally the energies [B] of the CURRENT
 * positions: (a) the second half-kick of the pending step, (b) when step % interval == 0 a log row and a frame of the now consistent (x, v, F), (c) this
 * step's noise, first half-kick and drift, pos32 = (float) r.  mode 0: velocity Verlet; mode 1: Langevin with friction fr (1/fs) at kT (Hartree), fix_com.
 * finish_only != 0: (a) and (b) only, the last call of a run; it advances nothing.  xi / eta (device f64[N][3], nullable, both or none): the normals of (c)
 * instead of the generator's.  Generator: Philox4x32-10 keyed by `seed`, counter (mol_key, step, atom inside the molecule, draw), Box-Muller in float64; the
 * second half-kick generates the step's numbers again.  dt <= 0, kT < 0, fr < 0: NQ_ERR_ARG.  Like nq_lbfgs_step the call repeats the dimensions; on a mismatch
 * with the header the kernel touches nothing but header word 1 (-2) and the call still returns NQ_OK.
 * nq_md_normals: out f64[N][3] = exactly the normals the kernels draw at (seed, step): draw 0 = xi, 1 = eta (Langevin step), 2 = zeta (velocity
 * initialisation, step 0), 3 = the unused partner of zeta; mol_ptr int32[B+1] and mol_key int64[B] (nullable: index) are DEVICE arrays.
 * Results are bitwise reproducible and do not depend on which other molecules share the batch. */
int nq_md_constants(double* kappa_kb_host);
size_t nq_md_state_bytes(int32_t N, int32_t B, int32_t log_cap, int32_t frame_cap, int32_t flags);
int nq_md_state_layout(int32_t N, int32_t B, int32_t log_cap, int32_t frame_cap, int32_t flags, size_t* offsets_host);
int nq_md_init(void* state, size_t state_bytes, const int32_t* mol_ptr_host, const int64_t* mol_key_host, const double* masses_host, const uint8_t* fixed_host,
               int32_t N, int32_t B, int32_t log_cap, int32_t frame_cap, int32_t flags, const void* pos, int32_t pos_f64, const double* vel, float* pos32,
               int32_t* n_small_host, void* stream);
int nq_md_init_velocities(void* state, int32_t N, int32_t B, int32_t n_small, int32_t log_cap, int32_t frame_cap, int32_t flags, double T_init, int64_t seed,
                          int32_t remove_translation, int32_t remove_rotation, void* stream);
int nq_md_step(void* state, int32_t N, int32_t B, int32_t n_small, int32_t log_cap, int32_t frame_cap, int32_t flags, const void* forces, int32_t forces_f64,
               const void* energies, int32_t energies_f64, float* pos32, int32_t mode, double dt, double kT, double fr, int32_t interval, int64_t seed,
               const double* xi, const double* eta, int32_t finish_only, void* stream);
int nq_md_normals(int64_t seed, int32_t step, int32_t draw, const int32_t* mol_ptr, const int64_t* mol_key, int32_t N, int32_t B, double* out, void* stream);

/* ---- Batched normal modes: finite-difference Hessians and a Jacobi eigensolver (csrc/vib.hip; entry points added, ABI 17 unchanged) ------------------------
 * Replaces: PYGAseInterface.compute_normal_modes (nablaDFT/optimization/pyg_ase_interface.py:317-334: ase.vibrations.Vibrations(atoms).run(), .summary(),
 * .write_jmol()).  ase is not in the reference tree: the arithmetic is restated (nabladft_amd/vibrations.py) and unpinned against ase.
 * Units: Hartree, Angstrom, amu; every array below is float64 unless said otherwise.  D = 3 x (free atoms of the batch), P = sum over molecules of m_b^2 with
 * m_b = 3 x (free atoms of molecule b) <= 576 (NQ_ERR_MOL_TOO_LARGE above); the caller computes both from mol_ptr and the fixed mask, nq_vib_init checks them.
 * The displacement list is molecule-major over (molecule, free degree of freedom); displacement j owns two images of its molecule, "-" then "+".
 * `state` is ONE caller-owned device buffer of nq_vib_state_bytes(N, B, D, P) bytes, 16-byte aligned (0 = bad dimensions, see nq_last_error).
 * nq_vib_state_layout fills offsets_host[18] with the byte offsets of: header int32[16] = {N, B, D, P low word, P high word, status (-2: a call came with other
 * dimensions than nq_vib_init and did nothing, -3: a chunk's image tensor has another size than the plan), n_lds}; mol_ptr int32[B+1]; dof_ptr int32[B+1];
 * hess_ptr int64[B+1] (start of each molecule's packed m_b x m_b matrices); order int32[B] (molecules whose matrix fits the LDS first); free_atom int32[D/3];
 * disp_mol int32[D]; disp_off int64[D+1] (atoms of all images before displacement j); im [D] = mass^-1/2 per degree of freedom; r [N][3] (the geometry);
 * h [D] (realised steps); asymmetry [B]; sweeps int32[B]; status int32[B] (0 converged, 1 sweep cap reached, 2 wrong launch plan); omega2 [D]; work [P];
 * hessian [P]; modes [P] (row k of a molecule's block = mode k, ascending omega2).
 * nq_vib_init: mol_ptr_host, masses_host (amu, every free atom's > 0) and fixed_host (nullable uint8[N]) are HOST arrays; copies `pos` (float32, or float64
 * when pos_f64) into r, writes plan_host[3] = {n_lds, largest m in LDS, largest m}, synchronises `stream` once.
 * nq_vib_displace: chunk [c0, c1) of the displacement list -> image_pos float32 [image_atoms][3], image_atoms = disp_off[c1] - disp_off[c0]: every image is
 * (float) r of its molecule with one coordinate (float)(r -+ delta); h[j] = (double) x32+ - (double) x32-, the step the quotient divides by.
 * nq_vib_accumulate: the model's forces on those images (float32, or float64 when forces_f64) -> rows (F- - F+)[free] / h[j] of `work`.
 * nq_vib_finish: hessian = (G + G^T) / 2, asymmetry = max |G - G^T| per molecule, work = im_i hessian_ij im_j (the mass-weighted matrix, exactly symmetric).
 * nq_vib_eigh: eigen-decomposition of every molecule's matrix in `work` (which it overwrites) by the parallel cyclic Jacobi method, one 256-thread workgroup
 * per molecule (round-robin ordering; the matrix in LDS when m <= 141, else in place in global memory); stops at off(A) <= m 2^-52 |A|_F or after 30 sweeps.
 * Writes omega2 ascending, modes (eigenvector k in row k, multiplied by im when scale_modes, orthonormal otherwise), sweeps and status.  n_lds, max_m_lds and
 * max_m are what nq_vib_init returned.  No atomics: results are bitwise reproducible and do not depend on which other molecules share the batch. */
size_t nq_vib_state_bytes(int32_t N, int32_t B, int32_t D, int64_t P);
int nq_vib_state_layout(int32_t N, int32_t B, int32_t D, int64_t P, size_t* offsets_host);
int nq_vib_init(void* state, size_t state_bytes, const int32_t* mol_ptr_host, const double* masses_host, const uint8_t* fixed_host, int32_t N, int32_t B,
                int32_t D, int64_t P, const void* pos, int32_t pos_f64, int32_t* plan_host, void* stream);
int nq_vib_displace(void* state, int32_t N, int32_t B, int32_t D, int64_t P, int32_t c0, int32_t c1, double delta, float* image_pos, int64_t image_atoms,
                    void* stream);
int nq_vib_accumulate(void* state, int32_t N, int32_t B, int32_t D, int64_t P, int32_t c0, int32_t c1, const void* forces, int32_t forces_f64,
                      int64_t image_atoms, void* stream);
int nq_vib_finish(void* state, int32_t N, int32_t B, int32_t D, int64_t P, void* stream);
int nq_vib_eigh(void* state, int32_t N, int32_t B, int32_t D, int64_t P, int32_t n_lds, int32_t max_m_lds, int32_t max_m, int32_t scale_modes, void* stream);

/* ---- Batched orbital energies: the generalized symmetric eigenproblem H C = S C diag(eps) (csrc/orbitals.hip, csrc/orbdens.hip; entry points added, ABI 17 unchanged) --------
 * Fills: the `orbital_energies` / `orbital_coefficients` slots that phisnet/nn/neural_network.py:969-993 returns as zeros (every entry point below serves
 * those lines), plus the HOMO / LUMO figures and the occupied-orbital errors the Hamiltonian papers report beside the matrix MAE.
 * Layout: B molecules, molecule b has m_b = orb_ptr[b+1] - orb_ptr[b] orbitals, 1 <= m_b <= 1024 (NQ_ERR_MOL_TOO_LARGE above, before any device work),
 * M = orb_ptr[B], and owns the m_b x m_b row-major block at pack_ptr[b] of every packed array, P = pack_ptr[B] = sum m_b^2 (BlockAssembler's pack_ptr /
 * mol_orb_ptr).  H and S are float32, or float64 when the flag beside them is set; only their lower triangles (j <= i) are read.  S = NULL: the identity
 * (the standard problem; the Cholesky and both triangular stages are skipped).  Every other array is float64 unless said otherwise.
 * `state` is ONE caller-owned device buffer of nq_orb_state_bytes(B, M, P) bytes, 16-byte aligned (0 = bad dimensions, see nq_last_error).
 * nq_orb_state_layout fills offsets_host[11] with the byte offsets of: header int32[16] = {B, M, P low word, P high word, status (-2: a call came with other
 * dimensions than nq_orb_init and did nothing; -3: a purification state met a call that reads coefficients, or the reverse), largest m, 2 once the state
 * holds a purification (below)}; orb_ptr int32[B+1]; pack_ptr int64[B+1]; order int32[B] (largest molecule first); status int32[B]
 * (0 solved, 1 S is not positive definite, 2 QL reached 60 sweeps on one eigenvalue, 3 the molecule's orb_ptr entries in the state are no longer within
 * 1..1024 orbitals -- the buffer was overwritten after nq_orb_init, which refuses such a batch; nothing else of that molecule is touched); info int32[B] (status 1: the 1-based index of the pivot that was <= 0
 * or not finite); iters int32[B] (QL sweeps); eps [M] (ascending inside each molecule); coeff [P] (ROW k of a molecule's block = orbital k, C^T S C = I, the
 * largest-magnitude component of every orbital, the first on ties, positive); work [P]; chol [P] (the factor L of S = L L^T, lower triangle).
 * nq_orb_init: orb_ptr_host is a HOST array [B+1]; checks it against M and P, builds pack_ptr and order, writes plan_host[2] = {largest m, LDS bytes of the
 * solve}, synchronises `stream` once.
 * nq_orb_solve: one launch, one 512-thread workgroup per molecule: Cholesky, A = L^-1 H L^-T symmetrised, Householder tridiagonalisation, implicit-shift QL
 * (deflation at |e_i| <= 2^-52 (|d_i| + |d_i+1|)), C = L^-T Y.  A molecule with status 1 gets NaN in eps and coeff; the others are untouched by it.  No
 * atomics: results are bitwise reproducible and do not depend on which other molecules share the batch.
 * nq_orb_frontier: n_occ int32[B] (device) -> homo = eps[n_occ - 1], lumo = eps[n_occ] (NaN when n_occ = m), gap = lumo - homo; all NaN for n_occ outside 1..m.
 * nq_orb_compare: a predicted against a target solution of the same batch (two states of the same dimensions, or the same state twice) under a common S ->
 * out [7][B]: mean |eps - eps^| over the occupied orbitals, the same over all orbitals, mean over the occupied orbitals of |c_k^T S c^_k|, |d homo|, |d lumo|,
 * |d gap|, min over the occupied orbitals of |c_k^T S c^_k|.  Overwrites the `work` part of state_pred (the full symmetric S).
 * nq_orb_wgram (csrc/orbdens.hip): the weighted Gram product of the coefficient rows a solve left in the state,
 *   out[pack_ptr[b] + i m_b + j] = sum_{k = lo_b .. hi_b - 1} w[orb_ptr[b] + k] C_b[k][i] C_b[k][j],
 * for one weight vector w0 [M] or two (w1 [M] -> out1, from the same operand loads); k_lo / k_hi int32 [B] on the device, NULL: 0 and m_b (values outside
 * 0..m_b are clamped); out0 / out1 [P], packed like coeff.  w = dL/d eps gives dL/dH and w = -eps dL/d eps gives dL/dS (d eps_k = c_k^T (dH - eps_k dS) c_k:
 * no difference of eigenvalues is divided by), both as the symmetric matrix sum_k g_k c_k c_k^T -- the gradient with respect to a symmetric input, the
 * convention of torch.linalg.eigh; w = 2 and w = 2 eps with k_hi = n_occ give the density matrix D and the energy-weighted density W.  One launch, one
 * workgroup per (molecule, 64 x 64 lower-triangle tile), v_mfma_f64_16x16x4_f64, no atomics; only j <= i is computed and written to (i, j) and (j, i): the
 * result is exactly symmetric, bitwise reproducible and independent of the rest of the batch.  A molecule with status != 0 gets NaN in its block, an empty
 * range zeros.  out1 is not touched when w1 is NULL; w1 without out1 is refused.
 * nq_orb_population (csrc/orbdens.hip): D [P] (a density matrix packed like coeff; any array of that layout) -> out_atom_pop [N] = sum over the atom's
 * orbitals of pop_mu = sum_nu D_mu,nu S_mu,nu (Mulliken), out_nelec [B] = sum_mu pop_mu = Tr(D S), out_eband [B] (NULL: skipped; needs H) = sum_mu,nu D_mu,nu
 * H_mu,nu = Tr(D H).  mol_ptr int32 [B+1] (atoms of molecule b) and atom_orb_ptr int64 [N+1] (first orbital of every atom, counted over the batch) are the
 * plan's mol_ptr / orb_ptr (nq_hblock_tables); an atom whose range leaves its molecule gets NaN.  Only the lower triangles of S and H are read; S = NULL: the
 * identity, pop = diag(D).  One workgroup per molecule, fixed summation orders, no atomics.
 * Both serve the same lines as the solver: they differentiate and post-process the `orbital_energies` / `orbital_coefficients` of neural_network.py:969-993.
 * The density response (csrc/orbresp.hip; entry points added, ABI 17 unchanged): the gradient of a loss on the closed-shell density D = 2 C_o C_o^T with respect to
 * H and S, as four products on the coefficient rows of the state.  n_occ int32 [B] (device; clamped to 0..m_b), occ_ptr int64 [B+1] (device) with
 * occ_ptr[b+1] - occ_ptr[b] >= n_occ_b m_b and O = occ_ptr[B] <= P: the "occupied-packed" layout of the caller-owned scratch arrays T, A_H, A_S ([m_b][n_occ_b]
 * row-major at occ_ptr[b]) and Rt_H, Rt_S ([n_occ_b][m_b]), O doubles each.  A block that does not lie inside [0, O) is not touched.
 *   nq_orb_resp_project: G [P] = dL/dD (need not be symmetric) -> Gs [P] = (G + G^T) / 2 (a scratch array, not G itself) and T = Gs C_o.
 *   nq_orb_resp_mo: W = C^T T -> A_H[k][i] = 4 W / (eps_i - eps_k) for k >= n_occ, 0 below; A_S[k][i] (NULL: skipped) = -eps_i A_H for k >= n_occ, -2 W below.
 *     The only division: by occupied-virtual differences.  Equal levels inside the occupied or inside the virtual orbitals are harmless; a vanishing
 *     HOMO-LUMO gap gives inf / NaN in that molecule's block only.
 *   nq_orb_resp_back: Rt_H[i][mu] = sum_k A_H[k][i] C[mu][k], and Rt_S from A_S (NULL: skipped) out of the same loads of the coefficients.  A_H must be
 *     zero over k < n_occ, as nq_orb_resp_mo writes it: without A_S the sum starts at the multiple of 4 below n_occ.
 *   nq_orb_syr2k: out[mu][nu] = 1/2 sum_{i < n_occ} (Rt[i][mu] C[nu][i] + C[mu][i] Rt[i][nu]) [P] for Rt0 and, from the same loads, Rt1 (NULL: skipped):
 *     Rt_H -> dL/dH, Rt_S -> dL/dS, symmetric matrices in the convention of nq_orb_wgram.  Lower-triangle 64 x 64 tiles mirrored: exactly symmetric.
 * All float64 on v_mfma_f64_16x16x4_f64, 64 x 64 output tiles, operands staged through LDS, the grid sized from (B, M, P), no atomics, a fixed summation order:
 * bitwise reproducible and independent of the rest of the batch.  status != 0: NaN in the molecule's own block of every output; n_occ = 0 or no virtual
 * orbital: zeros.  A second input without a second output is refused.
 * nq_orb_population_backward: the reverse of nq_orb_population.  g_pop [N], g_nelec [B], g_eband [B] (each NULL: zero) ->
 *   out_gD_ij = ((g_A(i) + g_A(j)) / 2 + g_nelec) S_ij + g_eband H_ij (S = NULL: the identity), and on request (NULL: skipped)
 *   out_gS_ij = ((g_A(i) + g_nelec) D_ij + (g_A(j) + g_nelec) D_ji) / 2 (needs S and D) and out_gH_ij = g_eband (D_ij + D_ji) / 2 (needs H and D):
 *   the gradients with respect to symmetric D, S and H, spread over both triangles; like the forward kernel only the lower triangles of S and H are read.
 * Fermi-Dirac smearing (csrc/orbsmear.hip, csrc/orbsmear_math.h; entry points added, ABI 17 unchanged): occupations F_k = 2 / (1 + exp((eps_k - mu) / kT)) with
 * mu fixed by sum_k F_k = n_elec, the density D = sum_k F_k c_k c_k^T (nq_orb_wgram with w0 = F) and its response to H and S over ALL orbital pairs, evaluated
 * without dividing by a difference of orbital energies: finite where levels coincide or cross.  n_elec, kT, mu, entropy float64 [B]; occ, docc, wdiag,
 * g_eps, g_occ float64 [M]; T, A_H, A_S, Rt_H, Rt_S float64 [P], packed like coeff ([m_b][m_b] row-major at pack_ptr[b]); all on the device.
 *   nq_orb_fermi: mu by a bracketed Newton iteration (bisection where Newton leaves the bracket; ends when the bracket is one ulp wide or sum F == n_elec),
 *     out_occ = F, out_docc = dF_k / d eps_k at fixed mu (<= 0), out_entropy = -2 sum (f ln f + (1 - f) ln(1 - f)), f = F / 2, 0 ln 0 = 0.  out_info int32 [B]:
 *     0 ok; 1: n_elec outside (0, 2 m), kT not a positive finite number (or >= 1e300), a non-finite eps or status != 0 -- that molecule's outputs are NaN.
 *   T = Gs C is nq_orb_resp_project with n_occ = m_b, occ_ptr = pack_ptr, O = P.
 *   nq_orb_smear_mo: W = C^T T [m][m]; off the diagonal A_H = K o W and A_S (NULL: skipped) = KS o W from the same accumulator, K_ij = (F_i - F_j) / (eps_i -
 *     eps_j) written as -(1 / (2 kT)) sinhc((x_i - x_j) / 2) / (cosh(x_i / 2) cosh(x_j / 2)), KS_ij = -((F_i + F_j) / 2 + (eps_i + eps_j) / 2 K_ij); wdiag = W_kk.
 *     The diagonals of A_H / A_S are not written.
 *   nq_orb_smear_diag: from wdiag, occ, docc and the upstream gradients g_eps [M], g_occ [M], g_mu [B], g_ent [B] (each NULL: zero):
 *     gF_k = g_occ_k + g_ent x_k + W_kk, e_k = g_eps_k + F'_k (gF_k - sum_j p_j gF_j) + p_k g_mu with p_k = F'_k / sum_j F'_j (evaluated as a softmax of
 *     -|x|: a sum of derivatives that underflows inside a wide gap divides nothing); A_H[k][k] = e_k, A_S[k][k] (NULL: skipped) = -eps_k e_k - F_k W_kk.
 *   nq_orb_smear_back: Rt_H[i][mu] = sum_k A_H[k][i] C[mu][k] over all k, and Rt_S from A_S (NULL: skipped) out of the same loads of the coefficients.
 *   dL/dH = C A_H C^T and dL/dS = C A_S C^T are nq_orb_syr2k on Rt_H / Rt_S with n_occ = m_b, occ_ptr = pack_ptr, O = P: exactly symmetric.
 * The products run on v_mfma_f64_16x16x4_f64 like the closed-shell chain's; no atomics, fixed summation orders, bitwise reproducible and independent of the
 * rest of the batch; status != 0: NaN in the molecule's own blocks.  A second input without a second output is refused.
 * Purification (csrc/orbpurify.hip; entry points added, ABI 17 unchanged): the closed-shell density D = 2 Z^T X Z and its gradients WITHOUT a solve, for the
 * quantities that need the occupied subspace only.  Z = L^-1 of S = L L^T, Ht = sym(Z H Z^T), X the projector on the n_occ lowest levels of Ht by second-order
 * spectral-projection purification (SP2): X_0 = (e_max I - Ht) / (e_max - e_min) from Gershgorin bounds, iteration k: Y = X X, t = tr X, t2 = tr Y,
 * delta_k = t - t2; stop with X = X_k when delta_k = 0, or when k >= 2 and |delta_k| >= |delta_k-1| and |delta_k-1| < 1e-6 max(1, n_occ); else X = Y if
 * |t2 - n_occ| <= |2 t - t2 - n_occ| (log entry 1), else X = 2 X - Y (log entry 2); the stopping iteration logs 3.  n_occ <= 0: X = 0; n_occ >= m or
 * e_max = e_min: X = I; neither iterates.  Not stopped after max_iter (1..10000) iterations: status 4, X = NaN.  Needs an open gap: a level shared by the
 * occupied and the virtual side does not converge.  No energies, no smearing, closed shells only.
 * Where things live: the state of nq_orb_init, whose parts `coeff` / `work` / `chol` hold X / Ht / Y (status 0, 1: the orthogonaliser failed on this
 * molecule, info = the 1-based pivot, 4: not converged; iters = the updates applied).  Caller-owned, float64 on the device: Z [P] (one orthogonaliser serves
 * any number of states of the same batch), X1, Q, tmp, Gt [P], ctl [B][40 + max_iter] = {e_min, e_max, kind (0 iterates, 1 X = 0, 2 X = I), n_occ, tr X and
 * tr Y of the last iteration, 0, 0, 16 slots (partial tr X, partial tr Y) of the diagonal 64 x 64 tiles, delta_k of every iteration} and log int32
 * [B][max_iter].  The first call of nq_orb_pur_orthogonalizer / nq_orb_pur_init marks the state for good (header word 6 = 2): from then on nq_orb_wgram, the
 * response and the smear families refuse it, and the step / run / response entry points below refuse a state without the mark: header status -3, nothing touched.
 *   nq_orb_pur_orthogonalizer: S (lower triangle, float32 or float64) -> Z [P], lower triangular, the upper triangle written as zero; the Cholesky stage has
 *     the arithmetic and the pivot rule of nq_orb_solve; a failed molecule: status 1, info, its block of Z NaN, the others intact.  Latency-bound; call it once
 *     per batch and reuse Z.
 *   nq_orb_pur_congruence: out = alpha sym(Z A Z^T) (trans = 0) or alpha sym(Z^T A Z) (trans != 0) as two triangular products on the matrix cores, contraction
 *     ranges cut to the non-zero part of Z; "sym": the lower-triangle 64 x 64 tiles are computed and mirrored.  A [P] float32 / float64 (a_f64) is first made
 *     symmetric: its lower triangle mirrored (a_sym = 0) or (A + A^T) / 2 (a_sym != 0).  tmp [P]: the first product (A Z^T or A Z).  Z = NULL: out = alpha A
 *     made symmetric, tmp unused.  Uses the layout of the state only.  A, Z, tmp and out must be different arrays.
 *   nq_orb_pur_gemm: out = alpha A B + beta C (C = NULL: skipped), full m x m blocks [P]; the general products of the S half of the gradient.
 *   nq_orb_pur_init: Ht [P] (lower triangle, float32 / float64; NULL: what nq_orb_pur_congruence left in the `work` part) -> the bounds, X_0 and the trivial
 *     cases; clears ctl and log.  Z (NULL: none): a molecule whose block of Z starts with NaN gets status 1.  n_occ int32 [B] on the device.
 *   nq_orb_pur_step: exactly one iteration, number k (0-based, in order); nq_orb_pur_run: iterations 0 .. max_iter - 1 and the status-4 sweep, enqueued with
 *     no host round trip; the workgroups of a finished, trivial or failed molecule exit at once.
 *   Gradient for an upstream G = dL/dD: Gt = nq_orb_pur_congruence(Z, trans = 0, G, a_sym = 1, alpha = 2), then
 *   nq_orb_pur_response_init: X = X_0 again, X1 = -Gt / (e_max - e_min) (trivial molecule: X1 = 0, failed: NaN);
 *   nq_orb_pur_response_step / _run: along the logged branches Y = X X and Q = X1 X + X X1 from the same staged tiles, (X, X1) = (Y, Q) or
 *     (2 X - Y, 2 X1 - Q): the X sequence is the forward's bit for bit, nothing is decided and nothing divided.  With g = the final X1:
 *     dL/dH = sym(Z^T g Z) and dL/dS = -sym(Z^T (M + M^T + X Gt X) Z), M = g X Ht (nq_orb_pur_gemm, nq_orb_pur_congruence with a_sym = 1, alpha = -1),
 *     symmetric matrices in the convention of nq_orb_wgram.  X1 without Q (the second output) is refused.
 * float64 throughout on v_mfma_f64_16x16x4_f64 through the tile routine of the response kernels (K tile 16, no deeper prefetch); no atomics, fixed summation
 * orders, bitwise reproducible and independent of the rest of the batch.
 * Bond orders (csrc/orbbond.hip; entry points added, ABI 17 unchanged): the Mayer bond-order table and the atomic valences of a closed-shell density D [P]
 * (carrying the factor 2) under S, and their reverse.  Atoms own contiguous orbital ranges: mol_ptr int32 [B+1] and atom_orb_ptr int64 [N+1] as for
 * nq_orb_population; molecule b owns the n_b^2 ordered atom pairs (A, B), A = B included, row-major at bond_ptr[b] (int64 [B+1] on the device, Q =
 * bond_ptr[B]: the ragged layout of the Graphormer3D pair_ptr).  Only the layout of the state is read: a solver state and a purification state serve alike.
 *   nq_orb_bond_product: out_P [P] = D S per molecule, the general m x m product (P is not symmetric); only the lower triangles of D and of S (float32 or
 *     float64 by s_f64) are read.  S = NULL: P = D made symmetric from its lower triangle (the Wiberg index of an orthogonal basis).
 *   nq_orb_bond_reduce: out_bond [Q], B_AB = sum_{mu in A, nu in B} P[mu][nu] P[nu][mu], one wavefront per pair A >= B, (A, B) and (B, A) written from the same
 *     number: exactly symmetric; out_valence [N] (NULL: skipped), V_A = sum_{B != A} B_AB.  An atom whose orbital range leaves its molecule or that has more than
 *     32 orbitals gives NaN for its row and column.  A molecule whose entries of mol_ptr / bond_ptr do not describe n_b^2 entries inside [0, Q) is not touched.
 *   nq_orb_bond_backward: gB [Q], gV [N] (each NULL: zero) -> E [P] (caller-owned scratch, written first by an elementwise launch):
 *     E[mu][nu] = (Gamma_A(mu)A(nu) + Gamma_A(nu)A(mu)) P[nu][mu] = dL/dP with Gamma_AB = gB_AB + (A != B ? gV_A : 0); then out_gD = sym(E S) = 1/2 (E S + S E^T)
 *     (S = NULL: sym(E)) and out_gS = sym(D E) = 1/2 (D E + E^T D) (each NULL: skipped; out_gS needs S and D, and D is passed only with out_gS), the gradients
 *     with respect to symmetric D and S spread over both triangles, lower-triangle 64 x 64 tiles mirrored: exactly symmetric.  An orbital no valid atom owns
 *     carries NaN.
 * Löwdin analysis (csrc/orblowdin.hip; entry points added, ABI 17 unchanged): A = S^(1/2) and A^- = S^(-1/2), the congruences A D A and A^- H A^- and the
 * reverse of both, after a STANDARD solve of S itself (nq_orb_solve with H = S and S = NULL: eps = s, row k of coeff = u_k, S = U diag(s) U^T).
 *   nq_orb_low_weights: out_half [M] = a_k = sqrt(s_k), out_inv_half [M] = 1 / a_k, out_cond [B] = s_max / s_min, one workgroup per molecule.  A molecule with
 *     status != 0, a non-finite s_k or s_min <= 0 gets out_info [B] = 1 and NaN in all of its outputs (0 otherwise).  A and A^- [P] are then ONE nq_orb_wgram
 *     launch with w0 = out_half and w1 = out_inv_half.  Reads eps: a purification state is refused (header status -3).
 *   nq_orb_low_product: out_Y [P] = M X per molecule, the general m x m product of two symmetric operands; only the lower triangles of Msym (float32 or float64
 *     by m_f64) and of X (float64) are read.  The product loop is nq_orb_bond_product's.  Only the layout of the state is read.
 *   nq_orb_low_symprod: out [P] = alpha sym(X E) = alpha / 2 (X E + E^T X) (side 0) or alpha sym(E X) = alpha / 2 (E X + X E^T) (side 1); E [P] any matrix, X [P]
 *     symmetric, its lower triangle read; lower-triangle 64 x 64 tiles mirrored: exactly symmetric.  Only the layout of the state is read.  With Y = M X:
 *     M^L = X M X = symprod(Y, X, 0, 1); for a symmetric G = dL/dM^L: dL/dM = symprod(G X, X, 0, 1), dL/dX = Y G + G Y^T = symprod(Y, G, 1, 2).
 *   nq_orb_low_symmetrize: out [P] = (G + G^T) / 2 per molecule, G [P] any matrix, lower-triangle tiles mirrored: exactly symmetric; what makes an upstream
 *     gradient fit for the two launches above, on the device.  Only the layout of the state is read.
 *   nq_orb_low_mo: A_out [P] = K o (U^T T), the diagonal included, T [P] = g U as nq_orb_resp_project leaves it over all orbitals (n_occ = m, occ_ptr =
 *     pack_ptr, O = P); kind 0: K_ij = 1 / (a_i + a_j) (the reverse of S^(1/2)), kind 1: K_ij = -1 / (a_i a_j (a_i + a_j)) (of S^(-1/2)), a = sqrt(eps)
 *     recomputed from the state: no difference of eigenvalues is divided.  dL/dS = U A_out U^T is then nq_orb_smear_back (A_S = NULL) and nq_orb_syr2k over all
 *     orbitals.  A molecule nq_orb_low_weights would flag gets NaN.  Reads eps and coeff: a purification state is refused (header status -3).
 * SCF residual (csrc/orbcomm.hip; entry points added, ABI 17 unchanged): the commutator R^L = [H^L, D^L] of the Löwdin Hamiltonian and density above, which is
 * H D S - S D H in that basis and vanishes exactly when D is a stationary density of H; for an idempotent closed-shell D, sum R^L_ij^2 = 8 sum_{i occ, a virt} h_ia^2.
 *   nq_orb_comm_product: out [P] = alpha (X Y - Y X) per molecule.  Y [P] symmetric, its lower triangle read.  x_anti 0: X symmetric (lower triangle read), out
 *     ANTISYMMETRIC with a +0.0 diagonal; x_anti 1: X antisymmetric (STRICT lower triangle read, the mirrored element is the negated one, the stored diagonal
 *     is ignored), out SYMMETRIC.  Lower-triangle 64 x 64 tiles, each entry computed once and stored twice: exactly (anti)symmetric.  For C = X Y - Y X with
 *     symmetric X, Y and G_a = antisymmetrize(dL/dC): dL/dX = comm_product(G_a, 1, Y, +1), dL/dY = comm_product(G_a, 1, X, -1), both symmetric.
 *   nq_orb_comm_antisymmetrize: out [P] = (G - G^T) / 2 per molecule, G [P] any matrix, lower-triangle tiles mirrored: exactly antisymmetric, +0.0 diagonal.
 *   nq_orb_comm_norms: out_sumsq [B] = sum_ij R_ij^2 and out_maxabs [B] = max_ij |R_ij| (the DIIS error) over the whole m x m block of R [P], one workgroup per
 *     molecule, fixed order; a NaN entry gives NaN in both.
 *   All three read only the layout of the state (a solver state and a purification state serve alike) and refuse aliased outputs on the host.
 * All float64 on v_mfma_f64_16x16x4_f64 through the tile routine of the response kernels, the grids sized from (B, M, P), no atomics, fixed summation orders:
 * bitwise reproducible and independent of the rest of the batch.  status != 0: NaN in the molecule's own blocks of every output.
 * Square roots without a decomposition (csrc/orbsqrt.hip; entry points added, ABI 17 unchanged): A = S^(1/2) and A^- = S^(-1/2) by the coupled Newton-Schulz
 * iteration.  c = the largest absolute row sum of S (>= s_max), Y_0 = S / c, Z_0 = I; iteration k: T = (3 I - sym(Z Y)) / 2 (lower-triangle tiles of Z Y
 * mirrored), delta_k = m - tr(Z Y); stop with (Y, Z) = (Y_k, Z_k) when delta_k = 0, or when k >= 1 and |delta_k| < 1e-9 m and |delta_k| >= |delta_k-1|; else
 * Y' = Y T, Z' = T Z as full general products (log entry 1; the stopping iteration logs 3).  Y and Z are NOT symmetrised between iterations: doing so makes
 * the iteration diverge once it has reached its rounding floor.  A = sqrt(c) Y, A^- = Z / sqrt(c), the lower triangles mirrored.  About 18 iterations at
 * kappa_2(S) = 1e4, 32 at 1e8, which is the limit the stopping rule is meant for; an indefinite S never stops.
 * Where things live: the state of nq_orb_init supplies the layout and the words status (0, 1: c not finite or <= 0, 4: not stopped after max_iter
 * iterations, info = 1), info and iters (the updates applied); its P-sized parts are neither read nor written, so the state is not marked and any state of the
 * batch serves.  Caller-owned, float64 on the device: Y, Z, T, Y2, Z2 [P each; iteration k reads the pair k & 1 -- (Y, Z) is pair 0 -- and writes the other, so
 * an output never aliases an operand of its launch], ctl [B][24 + max_iter] = {c, sqrt(c), tr(Z Y) of the last iteration, 0 x 5, 16 slots (partial tr(Z Y) of
 * the diagonal 64 x 64 tiles), delta_k of every iteration} and log int32 [B][max_iter].
 *   nq_orb_sqrt_init: S (lower triangle, float32 or float64; the upper triangle is not read) -> c, Y_0, Z_0 into (Y, Z); clears ctl and log, sets status.
 *   nq_orb_sqrt_step: exactly one iteration, number k (0-based, in order: iteration k of a molecule runs only if k = 0 or log[k - 1] is an update), two
 *     launches; nq_orb_sqrt_run: iterations 0 .. max_iter - 1 (1..10000) enqueued with no host round trip; the workgroups of a finished or failed molecule
 *     exit at once.
 *   nq_orb_sqrt_finish: half [P] = sqrt(c) Y and inv_half [P] = Z / sqrt(c) from the pair the last update wrote, lower triangles mirrored: exactly symmetric.
 *     A molecule with status 1, or whose last log entry is an update (status 4, info 1 from here on), gets NaN in its own blocks of both; the others are
 *     untouched by it.
 *   NULL or aliased arrays, max_iter or k out of range and impossible dimensions are refused on the host and touch nothing.  float64 on
 *   v_mfma_f64_16x16x4_f64, no atomics, fixed summation orders: bitwise reproducible and independent of the rest of the batch; m = 1 .. 1024.
 * Frontier levels without a solve (csrc/orbfrontier.hip; entry points added, ABI 17 unchanged): HOMO and LUMO of the orthogonalised Hamiltonian Ht of a
 * purification (state part `work`) from its projector X (state part `coeff`) and its bounds shift [B][2] = (e_min, e_max) = ctl[b][0..1], by a Lanczos
 * recurrence on P (Ht - e_min I) P with P = X (side 0, HOMO) and on P (e_max I - Ht) P with P = I - X (side 1, LUMO); the projector is applied on both sides
 * of every application, every step is fully reorthogonalised in two passes.
 *   nq_orb_front_lanczos: one workgroup per (molecule, side).  Ht, X [P]: full symmetric blocks; n_occ int32 [B]; W_or_null [P]: the back-transform, a general
 *     block, coef_mu = sum_k W[k][mu] vec_k (the lower-triangular Z of nq_orb_pur_orthogonalizer or a symmetric S^(-1/2) alike; NULL: coef = vec); k_max in
 *     1..1024; tol in (0, 1); V: workspace of 2 sum_b min(m_b, k_max) m_b doubles behind vptr int64 [B+1] (side s of molecule b at vptr[b] + s min(m, k_max) m).
 *     Start vector v_0 = P r / |P r|, r_i = 0.5 + ((2654435761 i + 12345) mod 2^32) / 2^32 with i the orbital's index inside the molecule.  A side stops when
 *     beta_j |s_last| <= tol (e_max - e_min) for the top Ritz pair (theta, s) of the tridiagonal, or after min(m, k_max) steps.  Outputs: eps [B][2] (the
 *     Rayleigh quotient of the unshifted Ht, not theta), vec [2][M] (normalised), coef [2][M], iters int32 [B][2] (steps taken), res [B][2] (beta_j |s_last|
 *     at the stop), conv int32 [B][2]: 1 converged, 0 not converged, -1 the level does not exist (HOMO for n_occ <= 0, LUMO for n_occ >= m).  conv != 1, a
 *     molecule with status != 0 (conv 0) or a workspace slice that is too small (conv 0): NaN in that side's own eps, res, vec and coef, nothing else.
 *   nq_orb_front_gram: out_gH [P] = sum_side g[b][side] c c^T and out_gS_or_null [P] = -sum_side g[b][side] eps[b][side] c c^T for c = coef of the side
 *     (d eps / dH = c c^T, d eps / dS = -eps c c^T: the convention of the solver's energies); full blocks, exactly symmetric, elementwise.  conv = -1
 *     contributes 0; conv = 0 or status != 0: NaN in the molecule's blocks.  out_gS needs eps.
 *   NULL or aliased arrays, k_max, tol and impossible dimensions are refused on the host and touch nothing.  Plain float64 fma (memory-bound: no matrix-core
 *   instruction), no atomics, fixed summation orders: bitwise reproducible and independent of the rest of the batch; m = 1 .. 1024.  Only the layout and the
 *   status words of the state are read.
 * Occupied levels without a full solve (csrc/orbocc.hip; entry points added, ABI 17 unchanged): ALL occupied orbital energies and coefficients from the
 * projector X of a purification (state part `coeff`, kind "purification") and its orthogonalised Hamiltonian Ht (state part `work`).  An exact orthogonal
 * projector of rank n_occ has a pivoted Cholesky factor X = Q^T Q whose n_occ rows are orthonormal, so Rayleigh-Ritz on Hs = Q Ht Q^T gives the occupied levels
 * and C = V Q W their coefficients.  The stages, in order, with `occ` a second state of the batch as nq_orb_init left it (the results land in it) and `red` a
 * third, of B molecules with max(n_occ_b, 1) orbitals each (Mr orbitals, Pr packed entries):
 *   nq_orb_occ_factor(purification state): one workgroup per molecule, a left-looking pivoted Cholesky of X for exactly n_occ steps (n_occ int32 [B], clamped to
 *     0..m); the pivot is the largest remaining diagonal entry, the first on ties.  Outputs: Q [P] (rows 0 .. n_occ - 1 of a molecule's block, the other rows
 *     untouched; the entries of earlier pivots are exactly 0), pivots int32 [M] (-1 in the slots k >= n_occ), min_pivot [B] (+inf for n_occ = 0), defect [B]
 *     (the largest |left-over diagonal entry|), status int32 [B]: the state's own word where that is not 0 (1, 4), 5 for a pivot < 1 / (2 m) or not finite or a
 *     left-over diagonal entry >= 1 / (2 m) in magnitude (X is not a projector of rank n_occ: too few or too many pivots), else 0.  status != 0: NaN in the molecule's rows of Q, min_pivot and defect, -1 in its pivots; nothing else is touched.
 *     A state that holds no purification: header status -3.
 *   nq_orb_occ_reduce(occ, whose `coeff` is the Q of the factor): Hs = Q T for T = Ht Q^T, occupied-packed [m][n_occ] behind occ_ptr int64 [B+1] (O entries:
 *     what nq_orb_resp_project(occ, ..., G = Ht, Gs, T) forms), into the reduced packed layout red_ptr int64 [B+1] (R = Pr entries): n_occ x n_occ, lower
 *     triangle computed and mirrored (exactly symmetric); n_occ = 0: the 1 x 1 block [0]; status [B] (the factor's) != 0: a zero block.
 *   nq_orb_solve(red, Hs, float64, S = NULL): the standard problem of the reduced blocks.
 *   nq_orb_occ_back(occ, red): U [O] = V Q (V = the rows of red's `coeff`), C = U W for W_or_null [P] a general block, C[k][nu] = sum_mu U[k][mu] W[mu][nu] (the
 *     lower-triangular Z of nq_orb_pur_orthogonalizer or a symmetric S^(-1/2) alike; NULL: C = U), the solver's sign rule (the largest-magnitude component of
 *     every orbital positive, the first on ties); into occ: eps[k] = the reduced levels (ascending) and rows k of `coeff` for k < n_occ, NaN in every other
 *     eps slot and coefficient row of the molecule, so that nq_orb_wgram with k_hi = n_occ and nq_orb_compare (its occupied figures) run on occ unchanged.
 *     status int32 [B], in and out: the factor's word, else red's (2: the QL iteration of the reduced block did not converge) -- also written to occ's own
 *     status words; != 0: NaN in all the molecule's eps slots and coefficient rows.  A state that holds a purification: header status -3.
 *   NULL or aliased arrays, reduced dimensions that do not fit the batch and impossible dimensions are refused on the host and touch nothing.  float64; the
 *   products on v_mfma_f64_16x16x4_f64, the factor in plain fma (memory-bound); no atomics, fixed summation orders: bitwise reproducible and independent of the
 *   rest of the batch; m = 1 .. 1024, n_occ = 0 .. m.
 * Every call after nq_orb_init repeats the dimensions; on a mismatch the kernels do nothing and set the header status to -2. */
size_t nq_orb_state_bytes(int32_t B, int32_t M, int64_t P);
int nq_orb_state_layout(int32_t B, int32_t M, int64_t P, size_t* offsets_host);
int nq_orb_init(void* state, size_t state_bytes, const int32_t* orb_ptr_host, int32_t B, int32_t M, int64_t P, int32_t* plan_host, void* stream);
int nq_orb_solve(void* state, int32_t B, int32_t M, int64_t P, const void* H, int32_t h_f64, const void* S_or_null, int32_t s_f64, void* stream);
int nq_orb_frontier(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, double* out_homo, double* out_lumo, double* out_gap, void* stream);
int nq_orb_compare(void* state_pred, void* state_target, int32_t B, int32_t M, int64_t P, const void* S_or_null, int32_t s_f64, const int32_t* n_occ, double* out,
                   void* stream);
int nq_orb_wgram(void* state, int32_t B, int32_t M, int64_t P, const double* w0, const double* w1_or_null, const int32_t* k_lo_or_null, const int32_t* k_hi_or_null,
                 double* out0, double* out1_or_null, void* stream);
int nq_orb_population(void* state, int32_t B, int32_t M, int64_t P, const double* D, const void* H_or_null, int32_t h_f64, const void* S_or_null, int32_t s_f64,
                      int32_t N, const int32_t* mol_ptr, const int64_t* atom_orb_ptr, double* out_atom_pop, double* out_nelec, double* out_eband_or_null,
                      void* stream);
int nq_orb_resp_project(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* G, double* Gs,
                        double* T, void* stream);
int nq_orb_resp_mo(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* T, double* A_H,
                   double* A_S_or_null, void* stream);
int nq_orb_resp_back(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* A_H,
                     const double* A_S_or_null, double* Rt_H, double* Rt_S_or_null, void* stream);
int nq_orb_syr2k(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* Rt0,
                 const double* Rt1_or_null, double* out0, double* out1_or_null, void* stream);
int nq_orb_population_backward(void* state, int32_t B, int32_t M, int64_t P, const double* g_pop_or_null, const double* g_nelec_or_null,
                               const double* g_eband_or_null, const double* D_or_null, const void* H_or_null, int32_t h_f64, const void* S_or_null, int32_t s_f64,
                               int32_t N, const int32_t* mol_ptr, const int64_t* atom_orb_ptr, double* out_gD, double* out_gS_or_null, double* out_gH_or_null,
                               void* stream);
int nq_orb_fermi(void* state, int32_t B, int32_t M, int64_t P, const double* n_elec, const double* kT, double* out_mu, double* out_occ, double* out_docc,
                 double* out_entropy, int32_t* out_info, void* stream);
int nq_orb_smear_mo(void* state, int32_t B, int32_t M, int64_t P, const double* mu, const double* kT, const double* T, double* A_H, double* A_S_or_null,
                    double* wdiag, void* stream);
int nq_orb_smear_diag(void* state, int32_t B, int32_t M, int64_t P, const double* mu, const double* kT, const double* occ, const double* docc,
                      const double* wdiag, const double* g_eps_or_null, const double* g_occ_or_null, const double* g_mu_or_null, const double* g_ent_or_null,
                      double* A_H, double* A_S_or_null, void* stream);
int nq_orb_smear_back(void* state, int32_t B, int32_t M, int64_t P, const double* A_H, const double* A_S_or_null, double* Rt_H, double* Rt_S_or_null,
                      void* stream);
int nq_orb_pur_orthogonalizer(void* state, int32_t B, int32_t M, int64_t P, const void* S, int32_t s_f64, double* Z, void* stream);
int nq_orb_pur_congruence(void* state, int32_t B, int32_t M, int64_t P, const double* Z_or_null, int32_t trans, const void* A, int32_t a_f64, int32_t a_sym,
                          double alpha, double* tmp_or_null, double* out, void* stream);
int nq_orb_pur_gemm(void* state, int32_t B, int32_t M, int64_t P, const double* A, const double* Bm, const double* C_or_null, double alpha, double beta,
                    double* out, void* stream);
int nq_orb_pur_init(void* state, int32_t B, int32_t M, int64_t P, const void* Ht_or_null, int32_t h_f64, const double* Z_or_null, const int32_t* n_occ,
                    int32_t max_iter, double* ctl, int32_t* log, void* stream);
int nq_orb_pur_step(void* state, int32_t B, int32_t M, int64_t P, int32_t k, int32_t max_iter, double* ctl, int32_t* log, void* stream);
int nq_orb_pur_run(void* state, int32_t B, int32_t M, int64_t P, int32_t max_iter, double* ctl, int32_t* log, void* stream);
int nq_orb_pur_response_init(void* state, int32_t B, int32_t M, int64_t P, const double* Gt, int32_t max_iter, const double* ctl, double* X1, void* stream);
int nq_orb_pur_response_step(void* state, int32_t B, int32_t M, int64_t P, int32_t k, int32_t max_iter, const int32_t* log, double* Q, double* X1,
                             void* stream);
int nq_orb_pur_response_run(void* state, int32_t B, int32_t M, int64_t P, int32_t max_iter, const int32_t* log, double* Q, double* X1, void* stream);
int nq_orb_bond_product(void* state, int32_t B, int32_t M, int64_t P, const double* D, const void* S_or_null, int32_t s_f64, double* out_P, void* stream);
int nq_orb_bond_reduce(void* state, int32_t B, int32_t M, int64_t P, const double* Pm, int32_t N, int64_t Q, const int32_t* mol_ptr, const int64_t* atom_orb_ptr,
                       const int64_t* bond_ptr, double* out_bond, double* out_valence_or_null, void* stream);
int nq_orb_bond_backward(void* state, int32_t B, int32_t M, int64_t P, const double* gB_or_null, const double* gV_or_null, const double* Pm,
                         const double* D_or_null, const void* S_or_null, int32_t s_f64, int32_t N, int64_t Q, const int32_t* mol_ptr, const int64_t* atom_orb_ptr,
                         const int64_t* bond_ptr_or_null, double* E, double* out_gD_or_null, double* out_gS_or_null, void* stream);
int nq_orb_low_weights(void* state, int32_t B, int32_t M, int64_t P, double* out_half, double* out_inv_half, double* out_cond, int32_t* out_info, void* stream);
int nq_orb_low_product(void* state, int32_t B, int32_t M, int64_t P, const void* Msym, int32_t m_f64, const double* X, double* out_Y, void* stream);
int nq_orb_low_symprod(void* state, int32_t B, int32_t M, int64_t P, const double* E, const double* X, int32_t side, double alpha, double* out, void* stream);
int nq_orb_low_symmetrize(void* state, int32_t B, int32_t M, int64_t P, const double* G, double* out, void* stream);
int nq_orb_low_mo(void* state, int32_t B, int32_t M, int64_t P, int32_t kind, const double* T, double* A_out, void* stream);
int nq_orb_comm_product(void* state, int32_t B, int32_t M, int64_t P, const double* X, int32_t x_anti, const double* Y, double alpha, double* out, void* stream);
int nq_orb_comm_antisymmetrize(void* state, int32_t B, int32_t M, int64_t P, const double* G, double* out, void* stream);
int nq_orb_comm_norms(void* state, int32_t B, int32_t M, int64_t P, const double* R, double* out_sumsq, double* out_maxabs, void* stream);
int nq_orb_sqrt_init(void* state, int32_t B, int32_t M, int64_t P, const void* S, int32_t s_f64, int32_t max_iter, double* Y, double* Z, double* ctl, int32_t* log,
                     void* stream);
int nq_orb_sqrt_step(void* state, int32_t B, int32_t M, int64_t P, int32_t k, int32_t max_iter, double* Y, double* Z, double* T, double* Y2, double* Z2, double* ctl,
                     int32_t* log, void* stream);
int nq_orb_sqrt_run(void* state, int32_t B, int32_t M, int64_t P, int32_t max_iter, double* Y, double* Z, double* T, double* Y2, double* Z2, double* ctl, int32_t* log,
                    void* stream);
int nq_orb_sqrt_finish(void* state, int32_t B, int32_t M, int64_t P, int32_t max_iter, const double* Y, const double* Z, const double* Y2, const double* Z2,
                       const double* ctl, const int32_t* log, double* half, double* inv_half, void* stream);
int nq_orb_front_lanczos(void* state, int32_t B, int32_t M, int64_t P, const double* Ht, const double* X, const double* shift, const int32_t* n_occ,
                         const double* W_or_null, int32_t k_max, double tol, double* V, const int64_t* vptr, double* eps, double* vec, double* coef, int32_t* iters,
                         double* res, int32_t* conv, void* stream);
int nq_orb_front_gram(void* state, int32_t B, int32_t M, int64_t P, const double* g, const double* eps_or_null, const double* coef, const int32_t* conv, double* out_gH,
                      double* out_gS_or_null, void* stream);
int nq_orb_occ_factor(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, double* Q, int32_t* pivots, double* min_pivot, double* defect,
                      int32_t* status, void* stream);
int nq_orb_occ_reduce(void* state, int32_t B, int32_t M, int64_t P, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O, const double* T, const int32_t* status,
                      const int64_t* red_ptr, int64_t R, double* Hs, void* stream);
int nq_orb_occ_back(void* state, void* reduced_state, int32_t B, int32_t M, int64_t P, int32_t Mr, int64_t Pr, const int32_t* n_occ, const int64_t* occ_ptr, int64_t O,
                    const double* W_or_null, int32_t* status, double* U, void* stream);

/* ---- Graphormer3D building blocks (csrc/graphormer.hip; reference nablaDFT/graphormer/graphormer_3d.py) --------------------------------------------------
 * Ragged layout: atoms [N] behind ptr int32[B+1] (atom_mol int32[N] = molecule of each atom); molecule b owns the n_b^2 ordered pairs (i, j), i = j included,
 * row-major behind pair_ptr int64[B+1] (P = pair_ptr[B]).  "head-major" = per molecule [H][n][n] starting at H * pair_ptr[b]: the layout of the attention bias,
 * of its accumulated adjoint and of the uint8 dropout keep masks.  max_mol_atoms = the largest n_b of the batch, at most nq_g3d_max_mol_atoms() (above:
 * NQ_ERR_MOL_TOO_LARGE).  All sums have a fixed order (bitwise reproducible).
 * Pair featuriser (:126-146 GaussianLayer, :283-293): d = |pos_j - pos_i|, unit = (pos_j - pos_i) / (d + 1e-5), x = mul[64 z_i + z_j] d + bias[...],
 * gbf[p][k] = exp(-((x - means[k]) / s_k)^2 / 2) / (sqrt(2 * 3.14159) s_k), s_k = |stds[k]| + 1e-5; efeat[i] = sum_j gbf[(i, j)].  K <= 256; the caller
 * guarantees 0 < z < 64.  Backward: adjoints of means / stds [K] and mul / bias [4096] from grad_gbf [P][K] and / or grad_efeat [N][K] (either nullable; the
 * latter is broadcast over j in the kernel); order int64[P] = the pairs sorted by edge type, type_ptr int64[4097] = start of each type's run. */
int32_t nq_g3d_max_mol_atoms(void);
int nq_g3d_pair_forward(const float* pos, const int32_t* z, const int32_t* ptr, const int32_t* atom_mol, const int64_t* pair_ptr, const float* mul, const float* bias,
                        const float* means, const float* stds, int32_t N, int32_t K, int32_t max_mol_atoms, float* gbf, float* unit, float* dist, float* efeat,
                        void* stream);
size_t nq_g3d_pair_scratch_floats(int32_t N, int64_t P, int32_t K);
int nq_g3d_pair_backward(const float* pos, const int32_t* z, const int32_t* ptr, const int32_t* atom_mol, const int64_t* pair_ptr, const float* mul, const float* bias,
                         const float* means, const float* stds, const float* dist, const int64_t* order, const int64_t* type_ptr, int32_t N, int64_t P, int32_t K,
                         const float* grad_gbf, const float* grad_efeat, float* grad_means, float* grad_stds, float* grad_mul, float* grad_bias, float* scratch,
                         void* stream);
/* :300-303: attention bias [P][H] -> head-major and back (the adjoint of the first is the second). */
int nq_g3d_bias_to_heads(const float* pair_major, const int32_t* ptr, const int32_t* atom_mol, const int64_t* pair_ptr, int32_t N, int32_t H, float* head_major,
                         void* stream);
int nq_g3d_bias_from_heads(const float* head_major, const int32_t* ptr, const int32_t* atom_mol, const int64_t* pair_ptr, int32_t N, int32_t H, float* pair_major,
                           void* stream);
/* :40-59 SelfMultiheadAttention between in_proj and out_proj: qkv [N][3 H D] (q | k | v), D = 16 or 32; out [N][H D] = softmax((q scaling) k^T + bias)
 * (* keep_mask * mask_scale when keep_mask is given) v; lse [N][H] = row log-sum-exp.  Backward recomputes the probabilities from lse: grad_qkv [N][3 H D] is
 * written, grad_bias_heads (head-major) is ADDED TO in place; scratch: N * H floats. */
int nq_g3d_attention_forward(const float* qkv, const float* bias_heads, const uint8_t* keep_mask, float mask_scale, const int32_t* ptr, const int64_t* pair_ptr,
                             int32_t B, int32_t N, int32_t H, int32_t D, int32_t max_mol_atoms, float scaling, float* out, float* lse, void* stream);
int nq_g3d_attention_backward(const float* qkv, const float* bias_heads, const uint8_t* keep_mask, float mask_scale, const int32_t* ptr, const int64_t* pair_ptr,
                              int32_t B, int32_t N, int32_t H, int32_t D, int32_t max_mol_atoms, float scaling, const float* out, const float* lse,
                              const float* grad_out, float* grad_qkv, float* grad_bias_heads, float* scratch, void* stream);
/* :185-224 NodeTaskHead after q_proj / k_proj / v_proj (qkv [N][3 H D]): forces[i][c] = b3[c] + sum_h sum_j P_hij unit[(i, j)][c] (v_jh . W3[c][h D ..]),
 * W3 [3][H D] = force_proj{1,2,3}.weight, b3 [3] their biases; head_forces [N][H][3] and lse [N][H] are kept for the backward, which writes grad_qkv,
 * grad_W3, grad_b3 and adds to grad_bias_heads; scratch: nq_g3d_force_scratch_floats floats. */
int nq_g3d_force_forward(const float* qkv, const float* bias_heads, const uint8_t* keep_mask, float mask_scale, const float* unit, const float* W3, const float* b3,
                         const int32_t* ptr, const int64_t* pair_ptr, int32_t B, int32_t N, int32_t H, int32_t D, int32_t max_mol_atoms, float scaling,
                         float* head_forces, float* lse, float* forces, void* stream);
size_t nq_g3d_force_scratch_floats(int32_t N, int32_t H, int32_t D);
int nq_g3d_force_backward(const float* qkv, const float* bias_heads, const uint8_t* keep_mask, float mask_scale, const float* unit, const float* W3,
                          const int32_t* ptr, const int64_t* pair_ptr, int32_t B, int32_t N, int32_t H, int32_t D, int32_t max_mol_atoms, float scaling,
                          const float* head_forces, const float* lse, const float* grad_forces, float* grad_qkv, float* grad_bias_heads, float* grad_W3,
                          float* grad_b3, float* scratch, void* stream);
/* :111, :180 F.gelu (exact, erf) of x [rows][C] + bias [C] (nullable); backward: grad_x = grad_y gelu'(x + bias). */
int nq_g3d_gelu_forward(const float* x, const float* bias, int64_t rows, int32_t C, float* y, void* stream);
int nq_g3d_gelu_backward(const float* x, const float* bias, const float* grad_y, int64_t rows, int32_t C, float* grad_x, void* stream);
/* :311-312 energy_proj.layer2 (Linear C -> 1): y[r] = x[r] . w + b[0]; backward: grad_x [rows][C], grad_w [C], grad_b [1]; scratch:
 * nq_g3d_rowdot_scratch_floats floats. */
int nq_g3d_rowdot_forward(const float* x, const float* w, const float* b, int64_t rows, int32_t C, float* y, void* stream);
size_t nq_g3d_rowdot_scratch_floats(int64_t rows, int32_t C);
int nq_g3d_rowdot_backward(const float* x, const float* w, const float* grad_y, int64_t rows, int32_t C, float* grad_x, float* grad_w, float* grad_b, float* scratch,
                           void* stream);

/* ---- DimeNet++ building blocks (csrc/dimenet.hip; the core as restated in DESIGN_details.md) ----------------------------------------------------------------
 * Graph: CSR by target atom as nq_es_graph_* builds it (row_ptr int32[N+1], src / dst int32[E], sources ascending inside a row, geom [E][4] =
 * {pos[src] - pos[dst], |.|}) plus the edges sorted by source for the transposed walks (src_order int32[E], src_ptr int32[N+1]).  Edge (j->i) has d = |pos_i -
 * pos_j| and u = (pos_i - pos_j) / d; its triplets are the in-row of j without k = i (never stored).  All sums have a fixed order (bitwise reproducible).
 * Geometry: backward turns grad_d [E] / grad_u [E][3] (either nullable) into grad_vec [E][3] (scratch) and grad_pos [N][3]. */
int nq_dn_geom_forward(const float* geom, int64_t E, float* d, float* u, void* stream);
int nq_dn_geom_backward(const float* d, const float* u, const float* grad_d, const float* grad_u, const int32_t* row_ptr, const int32_t* src_order,
                        const int32_t* src_ptr, int32_t N, int64_t E, float* grad_vec, float* grad_pos, void* stream);
/* x = d / cutoff, env(x) = 1/x + a x^(p-1) + b x^p + c x^(p+1); rbf[e][n] = env sin(freq[n] x); rad[e][l][n] = env norms[l][n] j_l(roots[l][n] x), evaluated in
 * float64 (series below x = l, upward recurrence above) and rounded once; roots / norms: float64 [S][R].  S <= 8, R <= 16, 2 <= p <= 16.  Backward: grad_d [E] and
 * the per-edge rows grad_freq_rows [E][R] (their column sum is the gradient of freq); grad_rbf / grad_rad nullable. */
int nq_dn_basis_forward(const float* d, const float* freq, const double* roots, const double* norms, int64_t E, int32_t S, int32_t R, double cutoff,
                        int32_t envelope_p, float* rbf, float* rad, void* stream);
int nq_dn_basis_backward(const float* d, const float* freq, const double* roots, const double* norms, int64_t E, int32_t S, int32_t R, double cutoff,
                         int32_t envelope_p, const float* grad_rbf, const float* grad_rad, float* grad_d, float* grad_freq_rows, void* stream);
/* m[(j->i)][c] = sum over (k->j), k != i of x_kj[(k->j)][c] sum_b W_sbf2[c][b] sum_l Y_l(u_ji . u_kj) Q[(k->j)][l][b], Y_l = sqrt((2l+1) / 4 pi) P_l;
 * x_kj [E][I], Q [E][S][Bs], W_sbf2 [I][Bs]; I = 64, 128, 192 or 256, S <= 8, Bs <= 8.  Backward writes grad_x [E][I], grad_Q [E][S][Bs], grad_u [E][3] (both
 * edges of every triplet) and, unless it is NULL, grad_W_sbf2 [I][Bs]; scratch: nq_dn_triplet_scratch_floats floats (needed only with grad_W_sbf2). */
int nq_dn_triplet_forward(const float* x_kj, const float* Q, const float* u, const float* W_sbf2, const int32_t* row_ptr, const int32_t* src, const int32_t* dst,
                          int32_t E, int32_t I, int32_t S, int32_t Bs, float* m, void* stream);
size_t nq_dn_triplet_scratch_floats(int32_t E, int32_t I, int32_t Bs);
int nq_dn_triplet_backward(const float* x_kj, const float* Q, const float* u, const float* W_sbf2, const int32_t* row_ptr, const int32_t* src, const int32_t* dst,
                           const int32_t* src_order, const int32_t* src_ptr, int32_t E, int32_t I, int32_t S, int32_t Bs, const float* grad_m, float* grad_x,
                           float* grad_Q, float* grad_u, float* grad_W_sbf2, float* scratch, void* stream);
/* y = x * gate (elementwise, count floats) and its two adjoints. */
int nq_dn_gate_forward(const float* x, const float* gate, int64_t count, float* y, void* stream);
int nq_dn_gate_backward(const float* x, const float* gate, const float* grad_y, int64_t count, float* grad_x, float* grad_gate, void* stream);
/* out[i] = sum over the in-edges e of atom i of x[e] * gate[e] ([E][H] -> [N][H]). */
int nq_dn_gatesum_forward(const float* x, const float* gate, const int32_t* row_ptr, int32_t N, int32_t H, float* out, void* stream);
int nq_dn_gatesum_backward(const float* x, const float* gate, const float* grad_out, const int32_t* dst, int64_t E, int32_t H, float* grad_x, float* grad_gate,
                           void* stream);
/* Embedding block after its dense products: pre[e] = AB[dst[e]][:H] + AB[src[e]][H:] + Cr[e] + bias, y = silu(pre); AB [N][2H], Cr [E][H].  Backward: grad_pre
 * [E][H] (= the adjoint of Cr; its column sum is the adjoint of bias) and grad_AB [N][2H]. */
int nq_dn_embed_forward(const float* AB, const float* Cr, const float* bias, const int32_t* src, const int32_t* dst, int64_t E, int32_t H, float* pre, float* y,
                        void* stream);
int nq_dn_embed_backward(const float* pre, const float* grad_y, const int32_t* row_ptr, const int32_t* src_order, const int32_t* src_ptr, int32_t N, int64_t E,
                         int32_t H, float* grad_pre, float* grad_AB, void* stream);

/* ---- DimeNet++, second sweep (a loss on the forces: d loss / d parameters = -d/d parameters <v, dE/dpos>, v = d loss / d forces).  The adjoint that reaches the
 * first-backward node of a kernel is the kernel's tangent along a position displacement; the reverse of that tangent goes on to the parameters.  No adjoint of d, u
 * or the positions is formed.  A tangent argument that is NULL counts as zero (and gives the bits of a zero array).  Fixed summation order, no atomics.
 * geometry: w = tpos[dst] - tpos[src], td [E] = w . u, tu [E][3] = (w - (w . u) u) / d.
 * basis (float64 inside, rounded once): rbf_t [E][R] = t[e] drbf/dd, rad_t [E][S][R] = t[e] dRad/dd, freq_rows [E][R] = t[e] grad_rbf[e][n] d2rbf/(dd dfreq_n)
 * (grad_rbf nullable; the column sum of freq_rows is the adjoint of freq).
 * triplet forward: mt [E][I] = the tangent of nq_dn_triplet_forward along (tx [E][I], tQ [E][S][Bs], tu [E][3]), W_sbf2 fixed.  Triplet backward: the adjoints of
 * <g, mt> with respect to x_kj (a_x), Q (a_Q) and, unless NULL, W_sbf2 (a_W_sbf2; scratch: nq_dn_triplet_scratch_floats floats).  One launch each.
 * silu: a = the adjoint of g silu'(pre): a_g = a silu'(pre), a_pre = a g silu''(pre).
 * gate: the adjoints (a_gx, a_gg, either nullable) of nq_dn_gate_backward's outputs: a_g = a_gx gate + a_gg x, a_x = a_gg g, a_gate = a_gx g.
 * embed_scatter: out [N][2H] = {sum of rows [E][H] over the in-edges, sum over the out-edges} of every atom (the adjoint of the embedding block's gather). */
int nq_dnt_geom(const float* d, const float* u, const float* tpos, const int32_t* src, const int32_t* dst, int64_t E, float* td, float* tu, void* stream);
int nq_dnt_basis(const float* d, const float* freq, const double* roots, const double* norms, int64_t E, int32_t S, int32_t R, double cutoff, int32_t envelope_p,
                 const float* t, const float* grad_rbf, float* rbf_t, float* rad_t, float* freq_rows, void* stream);
int nq_dnt_triplet_forward(const float* x_kj, const float* Q, const float* u, const float* W_sbf2, const float* tx, const float* tQ, const float* tu,
                           const int32_t* row_ptr, const int32_t* src, const int32_t* dst, int32_t E, int32_t I, int32_t S, int32_t Bs, float* mt, void* stream);
int nq_dnt_triplet_backward(const float* x_kj, const float* Q, const float* u, const float* W_sbf2, const float* tx, const float* tQ, const float* tu,
                            const int32_t* row_ptr, const int32_t* src, const int32_t* dst, const int32_t* src_order, const int32_t* src_ptr, int32_t E, int32_t I,
                            int32_t S, int32_t Bs, const float* g, float* a_x, float* a_Q, float* a_W_sbf2, float* scratch, void* stream);
int nq_dnt_silu(const float* pre, const float* g, const float* a, int64_t count, float* a_g, float* a_pre, void* stream);
int nq_dnt_gate(const float* x, const float* gate, const float* g, const float* a_gx, const float* a_gg, int64_t count, float* a_g, float* a_x, float* a_gate,
                void* stream);
int nq_dnt_embed_scatter(const float* rows, const int32_t* row_ptr, const int32_t* src_order, const int32_t* src_ptr, int32_t N, int64_t E, int32_t H, float* out,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
