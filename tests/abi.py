"""Thin helper for the GPU tests: call C-ABI stage functions with torch tensors.

Every output buffer is a view into an allocation filled with NaN and followed by a NaN guard tail of GUARD elements:
an element the kernel does not write stays NaN and fails any `max |got - ref| <= tol` assertion, and a write past the
end of the output spoils the guard, which `Stages.check_guards()` reports.  The header describes every output of these
entry points as overwritten, not accumulated (e.g. include/dmpfold_hip.h: the backward outputs), so none is zero-filled.
"""
import ctypes as C

import numpy as np
import torch

from dmpfold2_amd import _lib
from dmpfold2_amd.predict import Engine


class Stages:
    def __init__(self, state_dict, max_L=128, max_N=512, device="cuda:0"):
        self.eng = Engine(device, max_L, max_N)
        self.eng.set_weights({k: torch.from_numpy(np.array(v)) for k, v in state_dict.items()})
        self.lib = self.eng.lib
        self.dev = self.eng.device
        self._guards = []              # (allocation, elements of the output) since the last check_guards()
        self._guard_bytes = 0

    def _s(self):
        return self.eng.stream()

    GUARD = 4096                       # elements of NaN after every output
    GUARD_PENDING_BYTES = 1 << 30      # outputs held for the guard check before one is made on the spot

    def poisoned(self, shape, dtype=torch.float32):
        """An output of `shape`: NaN, followed by a NaN guard tail of GUARD elements (checked by check_guards); for uint8
        (the winner buffers of the training slice) the poison and the guard are 0xFF."""
        n = 1
        for d in shape:
            n *= int(d)
        if self._guard_bytes > self.GUARD_PENDING_BYTES:
            self.check_guards()        # bound the memory held by tests that never check
        if dtype.is_floating_point:
            buf = torch.full((n + self.GUARD,), float("nan"), dtype=dtype, device=self.dev)
        else:                          # the winners (uint8): 0xFF is no winner, so an unwritten byte is visible too
            assert dtype == torch.uint8
            buf = torch.full((n + self.GUARD,), 0xFF, dtype=dtype, device=self.dev)
        self._guards.append((buf, n))
        self._guard_bytes += buf.numel() * buf.element_size()
        return buf[:n].view(shape)

    def f32(self, *shape):
        return self.poisoned(shape)

    def check_guards(self):
        """Wait for the queued work; every guard tail since the last check must still be NaN (0xFF after a uint8 output).
        Forgets those guards."""
        torch.cuda.synchronize(self.dev)
        guards, self._guards, self._guard_bytes = self._guards, [], 0
        for buf, n in guards:
            tail = buf[n:]
            bad = int((~torch.isnan(tail)).sum()) if tail.dtype.is_floating_point else int((tail != 0xFF).sum())
            assert bad == 0, f"{bad} of the {tail.numel()} guard elements after an output of {n} elements were written"

    def to(self, a, dtype=torch.float32):
        return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(self.dev).contiguous()

    def call(self, name, *args):
        conv = []
        for a in args:
            if isinstance(a, torch.Tensor):
                assert a.is_contiguous() and a.device.type == "cuda"
                conv.append(a.data_ptr())
            else:
                conv.append(a)
        rc = getattr(self.lib, name)(self.eng.ctx, *conv, self._s())
        _lib.check(rc)
        return rc

    # ---- stages ----------------------------------------------------------------------
    def msa_weights(self, alnmat):
        m = self.to(alnmat, torch.uint8)
        n, L = m.shape
        w = self.f32(n)
        self.call("dmp_msa_weights", m, n, L, w)
        return w

    def cov_build(self, alnmat, w):
        m = self.to(alnmat, torch.uint8)
        n, L = m.shape
        cov = self.f32(21 * L, 21 * L)
        self.call("dmp_cov_build", m, w, n, L, cov)
        return cov

    def spd_inverse(self, a):
        a = a.clone()
        self.call("dmp_spd_inverse", a, a.shape[0])
        return a

    def dca_contacts(self, inv, L):
        out = self.f32(L, L)
        self.call("dmp_dca_contacts", inv, L, out)
        return out

    def dca_features(self, alnmat):
        m = self.to(alnmat, torch.uint8)
        n, L = m.shape
        out = self.f32(L, L, 442)
        self.call("dmp_dca_features", m, n, L, out)
        return out

    def gru_vertical(self, alnmat):
        m = self.to(alnmat, torch.uint8)
        n, L = m.shape
        out = self.f32(L, 512)
        self.call("dmp_gru_vertical", m, n, L, out)
        return out

    def gru_vertical_group(self, alnmats):
        """dmp_gru_vertical_group with every member on this one context: the alignments' column tiles side by side in
        one chain of max N + 1 rows; one (L, 512) output per member.  Waits for the chain (the uploaded codes live here)."""
        k = len(alnmats)
        d = [self.to(m, torch.uint8) for m in alnmats]
        outs = [self.f32(m.shape[1], 512) for m in alnmats]
        ctxs = (C.c_void_p * k)(*[self.eng.ctx] * k)
        mp = (C.c_void_p * k)(*[x.data_ptr() for x in d])
        op = (C.c_void_p * k)(*[x.data_ptr() for x in outs])
        Ns = (C.c_int * k)(*[m.shape[0] for m in alnmats])
        Ls = (C.c_int * k)(*[m.shape[1] for m in alnmats])
        _lib.check(self.lib.dmp_gru_vertical_group(ctxs, k, mp, Ns, Ls, op, self._s()))
        torch.cuda.synchronize(self.dev)
        return outs

    def gru_bidir(self, which, x):
        T = x.shape[0]
        out = self.f32(T, 512)
        self.call("dmp_gru_bidir", which, x, T, out)
        return out

    def stem_static(self, mat1d, inv, contacts):
        L = mat1d.shape[1]
        z0 = self.f32(384, L, L)
        self.call("dmp_stem_static", mat1d, inv, contacts, L, z0)
        return z0

    def stem_update(self, z0, dmap):
        L = dmap.shape[0]
        x = self.f32(128, L, L)
        self.call("dmp_stem_update", z0, dmap, L, x)
        return x

    def conv(self, block, x):
        L = x.shape[-1]
        u = self.f32(128, L, L)
        st = self.poisoned((128, 2), torch.float64)
        self.call("dmp_block_conv5x5_maxout", block, x, L, u, st)
        return u, st

    def norm(self, block, u, st, x):
        L = x.shape[-1]
        out = self.f32(128, L, L)
        self.call("dmp_block_norm_scse_residual", block, u, st, x, L, out)
        return out

    def conv_bwd(self, block, x, du, idx=None):
        L = x.shape[-1]
        dx, dw, db = self.f32(128, L, L), self.f32(512, 128, 5, 5), self.f32(512)
        self.call("dmp_block_conv5x5_maxout_bwd", block, x, du, idx, L, dx, dw, db)
        return dx, dw, db

    def conv_winners(self, block, x):
        """the float32 forward of a training step: maxout output + the winner of every quadruple (uint8)"""
        L = x.shape[-1]
        u = self.f32(128, L, L)
        idx = self.poisoned((128, L, L), torch.uint8)
        self.call("dmp_block_conv5x5_maxout_winners", block, x, L, u, idx)
        return u, idx

    def norm_bwd(self, block, u, dout):
        L = u.shape[-1]
        du, dparams = self.f32(128, L, L), self.f32(2433)
        self.call("dmp_block_norm_scse_residual_bwd", block, u, dout, L, du, dparams)
        return du, dparams

    def stem_winners(self, z0, dmap):
        L = dmap.shape[0]
        u = self.f32(128, L, L)
        idx = self.poisoned((128, L, L), torch.uint8)
        self.call("dmp_stem_maxout_winners", z0, dmap, L, u, idx)
        return u, idx

    def stem_bwd(self, u, idx, dy, mat1d, dmap):
        L = dmap.shape[0]
        dw, dparams, dmat1d = self.f32(384, 955), self.f32(640), self.f32(512, L)
        self.call("dmp_stem_bwd", u, idx, dy, mat1d, dmap, L, dw, dparams, dmat1d)
        return dw, dparams, dmat1d

    def head_bwd(self, x, g):
        L = x.shape[-1]
        dx, dparams = self.f32(128, L, L), self.f32(258)
        self.call("dmp_head_conv_bwd", x, g, L, dx, dparams)
        return dx, dparams

    def head_gram(self, x):
        L = x.shape[-1]
        conf, M = self.f32(L), self.f32(L, L)
        self.call("dmp_head_gram", x, L, conf, M)
        return conf, M

    def trunk_pass(self, z0, dmap):
        L = dmap.shape[0]
        conf, M = self.f32(L), self.f32(L, L)
        self.call("dmp_trunk_pass", z0, dmap, L, conf, M)
        return conf, M

    def conv_ms(self, z0, dmap, passes=1):
        """Mean duration (ms) of the 5x5 convolution launches of `passes` trunk passes, from the HIP events the library
        records around every launch (dmp_profile_enable / dmp_profile_conv_intervals)."""
        L = dmap.shape[0]
        cap = 16 * passes
        _lib.check(self.lib.dmp_profile_enable(self.eng.ctx, 1, cap))
        for _ in range(passes):
            self.trunk_pass(z0, dmap)
        torch.cuda.synchronize()
        a, b, n = (C.c_float * cap)(), (C.c_float * cap)(), C.c_int()
        _lib.check(self.lib.dmp_profile_conv_intervals(self.eng.ctx, self.eng.ctx, a, b, cap, C.byref(n)))
        _lib.check(self.lib.dmp_profile_enable(self.eng.ctx, 0, 0))
        return sum(b[i] - a[i] for i in range(n.value)) / max(1, n.value)

    def eigh_top8(self, M):
        L = M.shape[0]
        out = self.f32(L, 8)
        self.call("dmp_eigh_top8", M, L, out)
        return out

    def coords_from_mds(self, mat1d, mds):
        L = mds.shape[0]
        ca = self.f32(L, 3)
        self.call("dmp_coords_from_mds", mat1d, mds, L, ca)
        return ca

    def pair_distances(self, ca, clamp=1):
        L = ca.shape[0]
        d = self.f32(L, L)
        self.call("dmp_pair_distances", ca, L, clamp, d)
        return d

    def refine(self, ca, steps):
        ca = ca.clone()
        self.call("dmp_refine_coords", ca, ca.shape[0], steps)
        return ca

    def backbone(self, ca, logit):
        L = ca.shape[0]
        coords, conf = self.f32(L, 5, 3), self.f32(L)
        self.call("dmp_ca_to_backbone", ca, logit, L, coords, conf)
        return coords, conf
