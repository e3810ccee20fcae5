"""TEST HELPERS — not part of the product, never imported by rcot_amd/.

Operations of whole-image inference that tests/host_double.py does not state on its own: the four-launch MDTA chain as
``TransformerBlockOp.forward`` wires it when ``attn_core_fwd`` declines (written against the backend interface, so the same function
runs on ``TorchDouble`` in fp64 / fp32 and on ``HipBackend``), and fp64 references of the per-pixel and stencil operations on SAMPLES of
tensors that are too large to evaluate whole (pixel columns for the 1x1 products, row bands with a one-row halo for the gate).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

# channels -> (heads, GDFN hidden width) of the four levels of the transport map (rcot_amd.params.ffn_hidden)
LEVEL = {48: (1, 127), 96: (2, 255), 192: (4, 510), 384: (8, 1021)}


def qkv_like(seeded_tensor, B, C, N, seed=1):
    """u = [q | k | v] with k = 0.5 q + noise: the Gram diagonal dominates, as it does in the network"""
    q, nz, v = (seeded_tensor(seed + i, (B, C, N)) for i in range(3))
    return torch.cat([q, 0.5 * q + nz, v], 1)


def mdta_chain(be, fast, heads, u, x, temp, WoT, sq, Graw, Gn, A, MfT, y):
    """row_sumsq, the Gram product over the pixels (dense into ``Graw``, and as the slabs the softmax kernel sums where the backend has
    them), attn_softmax, the fold of W_o into the attention matrix and the apply + residual: TransformerBlockOp.forward from
    ``be.row_sumsq`` to ``y``.  ``fast``: the apply goes to the K-major kernel (HipBackend.kmajor_worth of the block)."""
    B, C3, N = u.shape
    C = C3 // 3
    c = C // heads
    uu = u.view(B, 3, heads, c, N)
    Q, K, V = uu[:, 0], uu[:, 1], u.view(B, 3, C, N)[:, 2].unsqueeze(1)
    be.row_sumsq(u[:, :2 * C], sq)
    be.bmm_nt(Q, K, Graw)
    G = be.bmm_nt_slabs(Q, K)
    be.attn_softmax(Graw if G is None else G, sq, temp, Gn, A)
    woT = WoT.view(heads, c, C).unsqueeze(0).expand(B, -1, -1, -1)
    be.bmm_nn(A, woT, MfT.view(B, heads, c, C), transA=True)
    if fast:
        be.gemm_kmajor(MfT.unsqueeze(1), V, y.view(B, 1, C, N), C, C, R=x.view(B, 1, C, N))
    else:
        be.bmm_nn(MfT.unsqueeze(1), V, y.view(B, 1, C, N), transA=True, R=x.view(B, 1, C, N))


# ----------------------------------------------------------------------------- sampled references
def proj_columns(W, Xc, ln=None, R=None):
    """fp64 1x1 projection of the pixel columns ``Xc`` [Ci, n] (any device / dtype): W @ LN?(Xc) + R; with ``ln`` = (w, b) the
    WithBias-LayerNorm statistics are made here from the columns themselves.  Returns (Y [Co, n], mu [n], rstd [n])."""
    X = Xc.detach().double().cpu()
    mu = X.mean(0)
    rs = 1.0 / torch.sqrt(((X - mu) ** 2).mean(0) + 1e-5)
    if ln is not None:
        w, b = (t.detach().double().cpu() for t in ln)
        X = (X - mu) * rs * w[:, None] + b[:, None]
    Y = W.detach().double().cpu() @ X
    if R is not None:
        Y = Y + R.detach().double().cpu()
    return Y, mu, rs


def gate_rows(p, w, b, j, r0, r1):
    """fp64 gelu(dw3x3(p[b, j])) * dw3x3(p[b, j + hid]) on rows [r0, r1) of one plane of ``p`` [B, 2 hid, H, W], from a band with a
    one-row halo (the zero padding itself at the plane's top and bottom rows)"""
    hid, H = p.shape[1] // 2, p.shape[2]
    lo, hi = max(r0 - 1, 0), min(r1 + 1, H)
    band = torch.stack([p[b, j, lo:hi], p[b, j + hid, lo:hi]]).detach().double().cpu()
    band = F.pad(band, (0, 0, int(r0 == 0), int(r1 == H)))        # a halo row outside the plane is the zero padding
    k = torch.stack([w[j], w[j + hid]]).detach().double().cpu().view(2, 1, 3, 3)
    d = F.conv2d(band[None], k, padding=(0, 1), groups=2)[0]
    assert d.shape[1] == r1 - r0, (d.shape, r0, r1)
    return F.gelu(d[0]) * d[1]
