"""GPU numerics of the conv weight-gradient kernels' tile staging (csrc/wgrad.hip): the running (b, t)
tile bookkeeping, the per-wave DMA lists and the DMAs of tile t + 1 issued inside the MFMA steps of tile t.

Reference: the float64 weight / bias gradient of ``F.conv1d`` (torch.autograd.grad) on the values of the
bf16 inputs.  Bound: the suite's ``rel`` error < 1e-4, the bound test_hip_local_track.py already holds two
fp32 summation orders of this kernel to (the products of bf16 values are exact in fp32; what is left is the
fp32 accumulation over at most B * L = 4608 positions here, ~1e-6).

Shapes (B, L) of the wgrad2 cases, with the chunk count R = min(8, tiles) (``WGRAD_CU_EIGHTHS`` = 1 gives
the launcher's floor of 8 chunks on a 256-CU device, so that chunks hold several tiles; the default
setting, one tile per chunk at these sizes, runs as well):
  (2, 128)  one tile per sample, R clamps to 2: a chunk has no next tile to stage
  (3, 200)  a partial last tile (rows >= L from the zero block); R = 6, no multiple of 8: the plain id map
  (5, 330)  15 tiles in 8 chunks of 1-2 tiles that start mid-sample: the running (b, t) wraps inside a chunk
  (4, 512)  16 tiles, R = 8: two-tile chunks, both parities of the double buffer
  (9, 512)  R = 8, 4-5 tiles per chunk
Every configuration runs twice on the same inputs and must repeat bitwise (a staging race would not).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, KS, DIL, V = 128, 9, 5, 26
BOUND = 1e-4


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def conv_wgrad_f64(x, dy, d):
    """float64 dW [co][ci][k], db [co] of y = conv1d(x, W, b, 'same', dilation d) for upstream dy; x, dy [B, L, C]."""
    w = torch.zeros(C, C, KS, dtype=torch.float64, device=x.device, requires_grad=True)
    b = torch.zeros(C, dtype=torch.float64, device=x.device, requires_grad=True)
    y = F.conv1d(x.double().transpose(1, 2), w, b, padding=(KS // 2) * d, dilation=d)
    return torch.autograd.grad((y * dy.double().transpose(1, 2)).sum(), [w, b])


@functools.lru_cache(maxsize=None)
def case(B, L):
    """Inputs and float64 references of one shape, computed once and shared (never modified)."""
    g = torch.Generator(device="cuda").manual_seed(1000 * B + L)
    x, dn, dw = (torch.randn(B, L, C, device="cuda", generator=g).to(torch.bfloat16) for _ in range(3))
    return x, dn, dw, conv_wgrad_f64(x, dn, 1), conv_wgrad_f64(x, dw, DIL)


def zeros(n):
    return [(torch.zeros(C, C, KS, device="cuda"), torch.zeros(C, device="cuda")) for _ in range(n)]


def check(outs, refs, what):
    for i, ((dw, db), (rw, rb)) in enumerate(zip(outs, refs)):
        ew, eb = rel(dw, rw), rel(db, rb)
        print(f"{what} conv {i}: rel dW {ew:.2e} db {eb:.2e}")
        assert ew < BOUND and eb < BOUND, (what, i, ew, eb)


def assert_same(o1, o2):
    for (a, b), (c, d) in zip(o1, o2):
        assert torch.equal(a, c) and torch.equal(b, d)


@pytest.mark.parametrize("eighths", [1, None])
@pytest.mark.parametrize("B,L", [(2, 128), (3, 200), (5, 330), (4, 512), (9, 512)])
def test_wgrad2_vs_float64(B, L, eighths, monkeypatch):
    from proteinbert_pytorch_replication_amd.ops import local_track as lt
    if eighths is not None:
        monkeypatch.setattr(lt, "WGRAD_CU_EIGHTHS", eighths)
    x, dn, dw, ref_n, ref_w = case(B, L)
    runs = []
    for _ in range(2):
        outs = zeros(2)
        keep = lt._wgrad(dn, dw, x, KS, DIL, 2, B, L, outs)
        torch.cuda.synchronize()
        runs.append(outs)
    check(runs[0], [ref_n, ref_w], f"B={B} L={L} R={keep[0].shape[0]}")
    assert_same(*runs)


def test_wgrad2_single_conv(monkeypatch):
    from proteinbert_pytorch_replication_amd.ops import local_track as lt
    monkeypatch.setattr(lt, "WGRAD_CU_EIGHTHS", 1)
    B, L = 5, 330
    x, dn, _, ref_n, _ = case(B, L)
    runs = []
    for _ in range(2):
        outs = zeros(1)
        lt._wgrad(dn, None, x, KS, DIL, 1, B, L, outs)
        torch.cuda.synchronize()
        runs.append(outs)
    check(runs[0], [ref_n], "nconv=1")
    assert_same(*runs)


def test_wgrad2_halo_shards_vs_float64(monkeypatch):
    """pbx_wgrad2x on 3 shards of (3, 300) with 20 neighbour rows each side (zeros past the sequence ends),
    sliced as test_cp_halo_conv_kernels_match_whole_sequence does: the shards' sum is the whole gradient."""
    from proteinbert_pytorch_replication_amd.ops import local_track as lt
    monkeypatch.setattr(lt, "WGRAD_CU_EIGHTHS", 1)
    B, L, P, H = 3, 300, 3, 20
    Ls = L // P
    x, dn, dw, ref_n, ref_w = case(B, L)
    z = torch.zeros(B, H, C, dtype=x.dtype, device="cuda")
    xp = torch.cat([z, x, z], dim=1)
    runs = []
    for _ in range(2):
        outs = zeros(2)
        keep = []
        for r in range(P):
            sl = slice(r * Ls, (r + 1) * Ls)
            xe = xp[:, r * Ls:r * Ls + Ls + 2 * H].contiguous()
            keep += lt._wgrad(dn[:, sl].contiguous(), dw[:, sl].contiguous(), xe, KS, DIL, 2, B, Ls, outs, False, H, H)
        torch.cuda.synchronize()
        runs.append(outs)
    check(runs[0], [ref_n, ref_w], "halo shards")
    assert_same(*runs)


# (130, 330): 390 tiles on the kernel's cap of 256 workgroups -- chunks of 1-2 tiles that start mid-sample,
# so the next tile's DMAs inside the MFMA loop and the (b, t) wrap run (one tile per workgroup otherwise)
@pytest.mark.parametrize("B,L", [(3, 200), (5, 330), (130, 330)])
def test_wgrad_tok_vs_float64(B, L):
    from proteinbert_pytorch_replication_amd.ops import local_track as lt
    g = torch.Generator(device="cuda").manual_seed(7 * B + L)
    E = torch.randn(V, C, device="cuda", generator=g)
    # Token -1 is the kernel's "no token": what it stages itself for the positions >= L of a partial tile, a
    # position outside the sequence.  E[-1] is no embedding row, so the reference needs a meaning for it, and
    # takes the kernel's documented one: such a position has a zero input row and no conv output, hence no
    # upstream gradient (zero dpre rows, as the kernel stages them past L).  With live dpre rows there the
    # kernel's dW still matches (measured 8.5e-8 at (3, 200)) but its bias gradient, taken from the one-hot
    # sums of the centre tap, leaves those rows out (rel 0.20): tokens outside [0, V) are outside the
    # launcher's contract, in this commit as in its parent.
    tok = torch.randint(-1, V, (B, L), device="cuda", generator=g)
    tok[0, :3] = -1
    dn, dw = (torch.randn(B, L, C, device="cuda", generator=g).to(torch.bfloat16) for _ in range(2))
    xe = E.to(torch.bfloat16)[tok.clamp(min=0)]
    xe[tok < 0] = 0
    dn[tok < 0] = 0
    dw[tok < 0] = 0
    refs = [conv_wgrad_f64(xe, dn, 1), conv_wgrad_f64(xe, dw, DIL)]
    runs = []
    for _ in range(2):
        outs = zeros(2)
        lt._wgrad_tok(dn, dw, tok, E, DIL, B, L, outs)
        torch.cuda.synchronize()
        runs.append(outs)
    check(runs[0], refs, f"tok B={B} L={L}")
    assert_same(*runs)
