"""TEST INFRASTRUCTURE -- a small ctypes driver of the SchNet entry points (nq_schnet_workspace_bytes / _forward / _backward / _ws_lookup) for
tests/test_schnet_ops_gpu.py.  It owns the workspace and the gradient buffer and fills them with NaN before every forward / backward call: a sweep
that reads a slot before writing it, or a gradient row nobody writes, shows up as NaN instead of whatever the allocator left."""
import ctypes as C

import torch

from oracle import spk_schnet_ref as S

NAN = float("nan")
INT_BUFFERS = ("order", "pair_of", "pair_slot")


def schnet_cfg(F, L, R, cutoff, max_z):
    from nabladft_amd import _lib
    cfg = _lib.SchnetCfg()
    cfg.n_atom_basis, cfg.n_interactions, cfg.n_rbf, cfg.max_z = F, L, R, max_z
    width = float(torch.linspace(0.0, cutoff, R)[1].item())
    cfg.cutoff, cfg.rbf_coeff = float(cutoff), -0.5 / width ** 2
    return cfg


class Engine:
    def __init__(self, case, dev="cuda:0"):
        import nabladft_amd as nq
        from nabladft_amd import _lib
        self._lib, self.lib, self.case, self.dev = _lib, _lib.load(), case, dev
        c = case.cfg
        self.cfg = schnet_cfg(c.n_atom_basis, c.n_interactions, c.n_rbf, c.cutoff, c.max_z)
        self.shapes = S.schnet_param_shapes(c)
        P = S.make_schnet_params(c, case.param_seed)
        self.flat = torch.cat([P[k].reshape(-1) for k, _ in self.shapes]).to(dev)
        assert self.flat.numel() == self.lib.nq_schnet_num_params(C.byref(self.cfg))
        self.offsets = torch.linspace(0.0, c.cutoff, c.n_rbf).to(dev)
        self.nl = nq.build_neighbor_list(case.pos.to(dev), case.batch.to(dev), case.z.to(dev), c.cutoff, 2 ** 30)
        self.N, self.E, self.B = self.nl.N, self.nl.E, self.nl.B
        self.ws_bytes = int(self.lib.nq_schnet_workspace_bytes(C.byref(self.cfg), self.N, self.E, self.B))
        assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0
        self.ws = torch.empty(self.ws_bytes // 4, device=dev, dtype=torch.float32)
        self.energy = self.forces = self.grad = None

    def _nan(self, *shape):
        return torch.full(shape, NAN, device=self.dev, dtype=torch.float32)

    def forward_rc(self, want_forces=True):
        p, lib = self._lib.ptr, self.lib
        self.ws.fill_(NAN)
        self.energy, self.forces = self._nan(self.B), (self._nan(self.N, 3) if want_forces else None)
        rc = lib.nq_schnet_forward(C.byref(self.cfg), p(self.flat), p(self.offsets), C.byref(self.nl.c), p(self.ws), self.ws_bytes, p(self.energy),
                                   p(self.forces), self._lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def forward(self, want_forces=True):
        self._lib.check(self.forward_rc(want_forces))
        return self.energy, self.forces

    def backward_rc(self, grad_energy, grad_forces):
        p, lib = self._lib.ptr, self.lib
        self.grad = self._nan(self.flat.numel())
        rc = lib.nq_schnet_backward(C.byref(self.cfg), p(self.flat), p(self.offsets), C.byref(self.nl.c), p(self.ws), self.ws_bytes, p(grad_energy),
                                    p(grad_forces), p(self.grad), self._lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def backward(self, grad_energy, grad_forces):
        self._lib.check(self.backward_rc(grad_energy, grad_forces))
        return self.grad

    def mse_seeds(self, w_e=1.0, w_f=1.0):
        """dL/dE, dL/dF of L = w_e mse(E, y) + w_f mse(F, f_target) on the engine's own outputs."""
        y, ft = self.case.y.to(self.dev), self.case.ft.to(self.dev)
        ge = 2.0 * w_e * (self.energy - y) / self.B
        gf = None if self.forces is None else 2.0 * w_f * (self.forces - ft) / (3 * self.N)
        return ge, gf

    def train_step(self):
        self.forward(True)
        ge, gf = self.mse_seeds()
        return self.backward(ge, gf)

    def buf(self, name, layer=0, tangent=0):
        """Host copy of a named workspace buffer (flat): float32, or int32 for the index buffers."""
        off, cnt = C.c_size_t(), C.c_size_t()
        self._lib.check(self.lib.nq_schnet_ws_lookup(C.byref(self.cfg), self.N, self.E, self.B, name.encode(), layer, tangent, C.byref(off), C.byref(cnt)))
        assert (off.value + cnt.value) * 4 <= self.ws_bytes
        t = self.ws[off.value:off.value + cnt.value].cpu()
        return t.view(torch.int32) if name in INT_BUFFERS else t

    def grads(self, grad=None):
        """name -> host tensor, split from the flat gradient."""
        g = (self.grad if grad is None else grad).cpu()
        out, o = {}, 0
        for name, shape in self.shapes:
            n = 1
            for s in shape:
                n *= s
            out[name] = g[o:o + n].view(shape)
            o += n
        return out

    def graph(self, name):
        """Host copy of an array of the neighbour list (row_ptr, lowptr, col, dst, rev, geom)."""
        return self.nl.t[name].cpu()
