"""GPU numerics of the conv data gradient with the LayerNorm-1 finalize fused in (csrc/conv4.hip
``conv_dgrad4_kernel<true>``) at the sizes where the order of its staging loads can go wrong.

The staging pass prefetches the next trip of the wide tile while it converts this one, holds the narrow
tile's GELU' chunks in flight from the kernel's start and masks lanes by clamped loads and dropped buffer
stores instead of branches.  The cases:
  * (L, B) = (36, 2): one tile; both halos of both convolutions reach outside the sequence, fewer valid rows
    than one trip;
  * (130, 3): the second tile has 2 rows, so almost every load is clamped;
  * (257, 2): three tiles, a last tile of one row, odd L (a half LN1 position pair);
  * (512, 2): the workload's L.
Each is checked against the separate path (``ln1_finalize`` + ``conv_dgrad4_kernel<false>``, which shares no
staging code with the fused kernel) and against fp32 autograd of the same block (reference math:
ProteinBERT/modules.py:201-219), with the bounds of tests/test_hip_local_track.py
``test_dgrad_fin_matches_separate_finalize`` and tests/test_hip_numerics_elementwise.py.
"""
import functools

import pytest
import torch

from test_hip_local_track import make_block, rel, torch_local
from test_hip_numerics_elementwise import elementwise

pytestmark = pytest.mark.gpu

CASES = [(36, 2), (130, 3), (257, 2), (512, 2)]


def block_inputs(L, B):
    m, blk = make_block(L, seed=3)
    torch.manual_seed(L + B)
    x0 = torch.randn(B, L, 128, device="cuda").to(torch.bfloat16)
    gb0 = torch.randn(B, 128, device="cuda") * 0.5
    dh = torch.randn(B, L, 128, device="cuda")
    dv = torch.randn(B, 512, device="cuda") * 1e-2
    return blk, x0, gb0, dh, dv


def block_params(blk):
    return [blk.local_narrow_conv_layer[0].weight, blk.local_wide_conv_layer[0].weight, blk.local_norm_1.weight,
            blk.local_norm_1.bias, blk.local_linear_layer[0].weight]


def fused_grads(blk, x0, gb0, dh, dv, fin):
    from proteinbert_pytorch_replication_amd.ops import local_track
    old = local_track.DGRAD_FIN
    local_track.DGRAD_FIN = fin
    try:
        x = x0.clone().requires_grad_(True)
        gb = gb0.clone().requires_grad_(True)
        h2, vpart = local_track.local_block(x, gb, blk)
        loss = (h2.float() * dh).sum() + (vpart.sum(1) * dv).sum()
        out = torch.autograd.grad(loss, [x, gb] + block_params(blk))
        torch.cuda.synchronize()
    finally:
        local_track.DGRAD_FIN = old
    return [t.detach().clone() for t in out]


@functools.lru_cache(maxsize=None)
def case(L, B):
    """(separate path, fused, fp32 autograd) gradients of x, gb, Wn, Ww, g1, be1, Wl -- computed once per case."""
    blk, x0, gb0, dh, dv = block_inputs(L, B)
    sep = fused_grads(blk, x0, gb0, dh, dv, False)
    fin = fused_grads(blk, x0, gb0, dh, dv, True)
    xr = x0.float().clone().requires_grad_(True)
    gbr = gb0.clone().requires_grad_(True)
    rh2, rv = torch_local(xr, gbr, blk)
    ref = torch.autograd.grad((rh2 * dh).sum() + (rv * dv).sum(), [xr, gbr] + block_params(blk))
    torch.cuda.synchronize()
    return sep, fin, [t.detach().clone() for t in ref]


@pytest.mark.parametrize("L,B", CASES)
def test_fin_matches_separate_finalize(L, B):
    """The same dS1 formula and bf16 rounding on both paths: the block's gradients agree to the order of the
    dgb float atomics."""
    sep, fin, _ = case(L, B)
    for n, a, b in zip(["x", "gb", "wn", "ww", "g1", "be1", "wl"], sep, fin):
        e = rel(b, a)
        print(f"L={L} B={B} {n}: rel {e:.3e}")
        assert e < 2e-3, f"{n}: {e:.3e}"


@pytest.mark.parametrize("L,B", CASES)
def test_fin_elementwise_vs_fp32(L, B):
    """Per-element errors of dx, dgb and both conv weight gradients against fp32 autograd of ``torch_local``."""
    _, fin, ref = case(L, B)
    bounds = {"dx": (1.6e-2, 0.15), "dgb": (6e-3, 0.12), "dWn": (1.2e-2, 0.18), "dWw": (1.2e-2, 0.18)}
    for name, a, b in zip(bounds, fin, ref):
        nmax, p999 = elementwise(a, b)
        print(f"L={L} B={B} {name}: max|err|/max|ref| {nmax:.2e}  p99.9 rel {p999:.2e}")
        assert nmax < bounds[name][0] and p999 < bounds[name][1], (name, nmax, p999)


@pytest.mark.parametrize("L,B", CASES)
def test_fin_writes_every_output_once(L, B, monkeypatch):
    """The fused backward twice on the same inputs, dx / dpre_n / dpre_w filled with NaN before each launch: all
    three come back finite and the same bits both times (a dropped or misplaced store leaves NaN or differs)."""
    from proteinbert_pytorch_replication_amd.ops import local_track
    blk, x0, gb0, dh, dv = block_inputs(L, B)
    real = local_track.conv_dgrad_fin
    runs = []

    def poisoned(dh1, s1, st1, T1, BM1, sums1, TS1, g1, gdn, gdw, wtn, wtw, dx, dpn, dpw, dgb, *rest):
        for t in (dx, dpn, dpw):
            t.fill_(float("nan"))
        real(dh1, s1, st1, T1, BM1, sums1, TS1, g1, gdn, gdw, wtn, wtw, dx, dpn, dpw, dgb, *rest)
        runs.append([t.detach().clone() for t in (dx, dpn, dpw)])

    monkeypatch.setattr(local_track, "conv_dgrad_fin", poisoned)
    for _ in range(2):
        fused_grads(blk, x0, gb0, dh, dv, True)
    torch.cuda.synchronize()
    assert len(runs) == 2
    for name, a, b in zip(["dx", "dpre_n", "dpre_w"], *runs):
        assert a.shape == (B, L, 128)
        assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all(), name
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), name
