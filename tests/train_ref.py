"""Float64 reference of the training slice's backward (dmpfold2_amd/csrc/train.hip) with the maxout winners IMPOSED.

Built on the oracle's own functions (oracle/dmpfold_oracle.py: block_finish and head run unchanged on float64 tensors; the
stem is O.stem with its max replaced by the selection below) and on autograd.  torch.max routes a gradient to one
channel of a group, so two implementations of the same convolution that resolve a near-tie differently have different
- both valid - gradients (tests/test_gpu_train.py's docstring).  Here the maxout is a GATHER at winners the caller
gives, so the function is smooth in everything else and a kernel's backward can be compared at the winners the kernel's
own forward saved; whether those winners are right is a separate check (winner_margin).  With winners = None the
reference runs torch.max itself.

The arithmetic runs where the caller says (`device`).  The 5x5 convolution on a GPU is unfold + matmul in slabs of rows,
as _conv_f64 of tests/test_gpu_lengths.py (no float64 conv2d is assumed there); on the CPU it is F.conv2d.
tests/test_train_ref_cpu.py checks this module against the reference project's recorded autograd.
"""
import torch
import torch.nn.functional as F

import dmpfold_oracle as O

SLAB_PIXELS = 8192                   # pixels per im2col slab of the GPU form (3200 x 8192 doubles = 210 MB)


def conv5x5_unfold(x, w, b):
    """x (C, L, L), w (O, C, 5, 5), b (O) -> (O, L, L), padding 2: im2col slabs of whole rows + matmul (differentiable)"""
    L = x.shape[-1]
    w2 = w.reshape(w.shape[0], -1)
    xp = F.pad(x, (2, 2, 2, 2))
    rows = max(1, SLAB_PIXELS // L)
    out = []
    for lo in range(0, L, rows):
        hi = min(L, lo + rows)
        cols = F.unfold(xp[None, :, lo:hi + 4], 5)[0]                       # (25 C, (hi - lo) L)
        out.append((w2 @ cols + b[:, None]).reshape(w.shape[0], hi - lo, L))
    return torch.cat(out, 1)


def conv5x5(x, w, b):
    if x.is_cuda:
        return conv5x5_unfold(x, w, b)
    return F.conv2d(x[None], w, b, padding=2)[0]


def select(z, pool, winners):
    """z (128 pool, L, L) -> (128, L, L): channel winners[g][p] of every group, or (winners None) torch.max"""
    L = z.shape[-1]
    q = z.view(128, pool, L, L)
    if winners is None:
        return q.max(dim=1)[0]
    return q.gather(1, winners.to(z.device).long()[:, None])[:, 0]


def argmax_winners(z, pool):
    """the first maximal channel of every group (torch.argmax's rule), uint8 (128, L, L)"""
    L = z.shape[-1]
    return z.detach().view(128, pool, L, L).argmax(dim=1).to(torch.uint8)


def winner_margin(z, pool, winners):
    """How far below the group's maximum the chosen channel lies, in float64, at EVERY decision (0 where the choice is
    a maximal channel) -> (largest such margin, number of decisions that differ from the float64 argmax)."""
    L = z.shape[-1]
    q = z.detach().view(128, pool, L, L)
    w = winners.to(z.device).long()
    margin = q.max(dim=1)[0] - q.gather(1, w[:, None])[:, 0]
    return float(margin.max()), int((w != q.argmax(dim=1)).sum())


def route(du, pool, winners):
    """the dense gradient at the convolution's output: du at the winner of every group, 0 at the others"""
    L = du.shape[-1]
    dz = torch.zeros(128, pool, L, L, dtype=du.dtype, device=du.device)
    dz.scatter_(1, winners.to(du.device).long()[:, None], du[:, None])
    return dz.view(128 * pool, L, L)


def _f64(t, device):
    return torch.as_tensor(t).to(device).double()


NORM_PARAMS = ("layer1.norm.weight", "layer1.norm.bias", "scSE.cSE.fc.0.weight", "scSE.cSE.fc.2.weight",
               "scSE.sSE.conv.weight", "scSE.sSE.conv.bias")


def pack_dparams(grads):
    """the six parameter gradients of a block's second half in the layout of d_dparams (include/dmpfold_hip.h): 2433"""
    return torch.cat([g.reshape(-1) for g in grads])


def _block_params(W, k, device):
    p = f"resnet.{k}."
    return {n: _f64(v, device).requires_grad_(True) for n, v in W.items() if n.startswith(p)}


class Block:
    """Residual block k at input x (128, L, L): z = conv2d(x, W, b, padding 2) with its graph kept, so that the linear
    first half can be run backwards from several dz and the whole block from several winners."""

    def __init__(self, W, k, x, device="cpu"):
        self.k, self.P = k, _block_params(W, k, device)
        self.x = _f64(x, device).requires_grad_(True)
        self.w, self.b = self.P[f"resnet.{k}.layer1.lin.weight"], self.P[f"resnet.{k}.layer1.lin.bias"]
        self.z = conv5x5(self.x, self.w, self.b)

    def winners(self):
        return argmax_winners(self.z, 4)

    def u(self, winners):
        return select(self.z.detach(), 4, winners)

    def conv_bwd(self, du, winners):
        """the convolution half alone (linear in du): -> dx (128, L, L), dw (512, 128, 5, 5), db (512)"""
        dz = route(_f64(du, self.z.device), 4, winners)
        return torch.autograd.grad(self.z, (self.x, self.w, self.b), dz, retain_graph=True)

    def whole(self, dout, winners):
        """out = block_finish(select(z, winners), x), backwards from dout: -> dict u, out, du, dx (with the residual
        branch), dw, db, dparams (2433)"""
        u = select(self.z, 4, winners)
        out = O.block_finish(self.P, self.k, u[None], self.x[None])[0]
        norm = [self.P[f"resnet.{self.k}.{n}"] for n in NORM_PARAMS]
        g = torch.autograd.grad(out, [u, self.x, self.w, self.b] + norm, _f64(dout, out.device), retain_graph=True)
        return {"u": u.detach(), "out": out.detach(), "du": g[0], "dx": g[1], "dw": g[2], "db": g[3],
                "dparams": pack_dparams(g[4:])}


def norm_bwd(W, k, u, dout, device="cpu"):
    """the InstanceNorm + scSE + residual half alone, from a given u: -> du (128, L, L), dparams (2433)"""
    P = _block_params(W, k, device)
    u = _f64(u, device).requires_grad_(True)
    out = O.block_finish(P, k, u[None], torch.zeros_like(u)[None])[0]
    g = torch.autograd.grad(out, [u] + [P[f"resnet.{k}.{n}"] for n in NORM_PARAMS], _f64(dout, device))
    return g[0], pack_dparams(g[1:])


def stem_input(mat1d, f2d, dmap):
    """the 955-channel input as GRUResNet.forward builds it (Ref.resinp of tests/test_gpu_lengths.py): outer product of
    mat1d (512, L), the covariance + contact channels f2d (442, L, L), the distance channel dmap (L, L)"""
    pair = mat1d.unsqueeze(1) * mat1d.unsqueeze(2)
    return torch.cat((pair, f2d, dmap[None]), dim=0)[None]


def f2d_as_inverse(f2d):
    """the kernel's view of the covariance channels: inv[21 i + a][21 j + b] = f2d[21 a + b][i][j], and the contacts"""
    L = f2d.shape[-1]
    return f2d[:441].reshape(21, 21, L, L).permute(2, 0, 3, 1).reshape(21 * L, 21 * L).contiguous(), f2d[441].contiguous()


def stem_bwd(W, mat1d, f2d, dmap, dy, winners, device="cpu"):
    """resnet[0] (O.stem with the maxout as `select`) backwards from dy (128, L, L): -> dict z (384, L, L), u, y, du,
    dw (384, 955), db (384), dgamma, dbeta, dmat1d (512, L)"""
    P = {n: _f64(v, device).requires_grad_(True) for n, v in W.items() if n.startswith("resnet.0.")}
    m = _f64(mat1d, device).requires_grad_(True)
    inp = stem_input(m, _f64(f2d, device), _f64(dmap, device))
    z = F.conv2d(inp, P["resnet.0.lin.weight"], P["resnet.0.lin.bias"])[0]
    u = select(z, 3, winners)
    y = F.instance_norm(u[None], weight=P["resnet.0.norm.weight"], bias=P["resnet.0.norm.bias"], eps=1e-5)[0]
    g = torch.autograd.grad(y, [u, P["resnet.0.lin.weight"], P["resnet.0.lin.bias"], P["resnet.0.norm.weight"],
                                P["resnet.0.norm.bias"], m], _f64(dy, device))
    return {"z": z.detach(), "u": u.detach(), "y": y.detach(), "du": g[0], "dw": g[1].reshape(384, 955), "db": g[2],
            "dgamma": g[3], "dbeta": g[4], "dmat1d": g[5]}


def head_bwd(W, x, g, device="cpu"):
    """O.head (Conv2d 128 -> 2, kernel 1) backwards from the gradient at its two planes: -> dx, dparams (258)"""
    P = {n: _f64(W[n], device).requires_grad_(True) for n in ("resnet.17.weight", "resnet.17.bias")}
    x = _f64(x, device).requires_grad_(True)
    d = torch.autograd.grad(O.head(P, x[None])[0], [x, P["resnet.17.weight"], P["resnet.17.bias"]], _f64(g, device))
    return d[0], torch.cat((d[1].reshape(-1), d[2]))
