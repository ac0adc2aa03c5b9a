"""GPU: the inference heads (ops/infer_heads.py: csrc/infer.hip, EPI_GO_PROB in csrc/gemm.hip) alone, on random
bf16 encoder outputs built exactly as tests/test_hip_eval_heads.py builds them, against an fp64 CPU reference
from the same bf16 ``h`` / ``g`` and the bf16-rounded ``Wo`` / ``Wa``.

Probabilities: within 16 x the error of an independent fp32 torch evaluation (e_P relative for the local heads,
e_p for the GO head; 16 is the width test_hip_eval_heads.py grants ``__expf`` and the MFMA accumulation order)
plus 2^-24.  Calls: exact against the kernel's own stored probabilities (first maximal index).  Top-k: exact
against a CPU stable descending sort of the very matrix the kernel read.  Pool: the fp32 sequential-summation
bound against fp64.  Every launcher twice, bitwise equal."""
import functools

import pytest
import torch

from proteinbert_pytorch_replication_amd.models import ProteinBERT

pytestmark = pytest.mark.gpu

SHAPES = [(6, 24, 96), (17, 33, 96), (130, 37, 96), (300, 37, 8943), (1030, 9, 96)]
G = 256
V = 26
F64 = torch.float64
EPS = 2.0 ** -24
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def _case(B, L, A):
    """Inputs on the GPU (the same random stream as tests/test_hip_eval_heads.py::_case) and the fp64 CPU
    reference of both heads' probabilities, computed once per shape and only read."""
    torch.manual_seed(B + L)
    m = ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64, num_heads=4,
                    num_blocks=1, device="cuda", backend="hip")
    h = torch.randn(B, L, 128, device="cuda").to(torch.bfloat16)
    g_bf = torch.randn(B, G, device="cuda").to(torch.bfloat16)
    lo, go = m.pretraining_local_output[0], m.pretraining_global_output[0]
    c = dict(m=m, h=h, g_bf=g_bf, lo=lo, go=go)
    h64 = h.cpu().to(F64)
    wo = lo.weight.detach().to(torch.bfloat16).cpu()
    bo = lo.bias.detach().cpu()
    Z = h64 @ wo.to(F64).t() + bo.to(F64)
    Z32 = h.cpu().float() @ wo.float().t() + bo                    # the independent fp32 evaluation
    for name, dim in (("ref", 0), ("paper", -1)):
        P = torch.softmax(Z, dim=dim)
        P32 = torch.softmax(Z32, dim=dim)
        c[name] = dict(P=P, e_P=float(((P32.to(F64) - P).abs() / P).max()))
    wa = go.weight.detach().to(torch.bfloat16).cpu()
    ba = go.bias.detach().cpu()
    p = torch.sigmoid(g_bf.cpu().to(F64) @ wa.to(F64).t() + ba.to(F64))
    p32 = torch.sigmoid(g_bf.cpu().float() @ wa.float().t() + ba)
    c["e_p"] = float(((p32.to(F64) - p).abs() / p).max())
    c["p"] = p
    return c


@functools.lru_cache(maxsize=None)
def _go_probs(B, L, A):
    """The kernel's GO probabilities of a case (contiguous [B, A], on the GPU): the top-k tests' input."""
    from proteinbert_pytorch_replication_amd.ops.infer_heads import go_probs
    c = _case(B, L, A)
    return go_probs(c["g_bf"], c["go"].weight, c["go"].bias)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("B,L,A", SHAPES)
def test_go_probs(B, L, A):
    from proteinbert_pytorch_replication_amd.ops.infer_heads import go_probs
    c = _case(B, L, A)
    ld = (A + 4 + 3) // 4 * 4                                      # padded, 16-B rows: the vector-store path
    bufs = [torch.full((B + 1, ld), SENTINEL, device="cuda") for _ in range(2)]
    for buf in bufs:
        out = go_probs(c["g_bf"], c["go"].weight, c["go"].bias, out=buf[:B, :A])
        assert out.data_ptr() == buf.data_ptr()
    plain = _go_probs(B, L, A)                                     # ld = A (odd at A = 8943: scalar stores)
    torch.cuda.synchronize()
    assert torch.equal(_bits(bufs[0]), _bits(bufs[1]))             # bitwise repeatable
    got = bufs[0].cpu()
    assert (got[:B, A:] == SENTINEL).all() and (got[B] == SENTINEL).all()   # nothing outside [B, A] written
    assert torch.equal(_bits(got[:B, :A]), _bits(plain.cpu()))
    err = (got[:B, :A].to(F64) - c["p"]).abs()
    print(f"GO probs B={B} A={A}: e_p {c['e_p']:.3e} max err {float(err.max()):.3e} "
          f"worst err / e_p {float(err.max()) / c['e_p']:.2f} min p {float(c['p'].min()):.3e}")
    assert (err <= 16 * c["e_p"] + EPS).all()


@pytest.mark.parametrize("semantics", ["ref", "paper"])
@pytest.mark.parametrize("B,L,A", SHAPES)
def test_local_probs_and_calls(B, L, A, semantics):
    from proteinbert_pytorch_replication_amd.ops import infer_heads as ih
    c = _case(B, L, A)
    fn = ih.local_probs_ref if semantics == "ref" else ih.local_probs_paper
    w, b = c["lo"].weight, c["lo"].bias
    n = B * L * V
    bufs = [torch.full((n + 64,), SENTINEL, device="cuda") for _ in range(2)]
    res = [fn(c["h"], w, b, out=buf[:n].view(B, L, V)) for buf in bufs]
    Pn, tok_n, pmax_n = fn(c["h"], w, b, store_probs=False)
    torch.cuda.synchronize()
    (P, tok, pmax), (P2, tok2, pmax2) = res
    assert Pn is None and tok.dtype == torch.int32 and pmax.dtype == torch.float32
    assert torch.equal(_bits(bufs[0]), _bits(bufs[1])) and torch.equal(tok, tok2)     # bitwise repeatable
    assert torch.equal(_bits(pmax), _bits(pmax2))
    assert (bufs[0][n:] == SENTINEL).all() and not (bufs[0][:n] == SENTINEL).any()    # exactly [B, L, V] written
    # the calls: exact against the stored probabilities, with or without the store
    Pc, tokc, pmaxc = P.cpu(), tok.cpu().long(), pmax.cpu()
    assert torch.equal(tokc, Pc.argmax(-1))
    assert torch.equal(_bits(pmaxc), _bits(Pc.gather(-1, tokc.unsqueeze(-1)).squeeze(-1)))
    assert torch.equal(tok_n, tok) and torch.equal(_bits(pmax_n), _bits(pmax))
    ref = c[semantics]
    rel = (Pc.to(F64) - ref["P"]).abs() / ref["P"]
    print(f"local probs {semantics} B={B} L={L}: e_P {ref['e_P']:.3e} worst rel err {float(rel.max()):.3e} "
          f"worst err / e_P {float(rel.max()) / ref['e_P']:.2f} min P {float(ref['P'].min()):.3e}")
    assert ((Pc.to(F64) - ref["P"]).abs() <= 16 * ref["e_P"] * ref["P"] + EPS).all()


def _check_topk(P, k):
    """``row_topk(P, k)`` twice against the CPU stable descending sort of the same fp32 matrix."""
    from proteinbert_pytorch_replication_amd.ops.infer_heads import row_topk
    v, i = row_topk(P, k)
    v2, i2 = row_topk(P, k)
    torch.cuda.synchronize()
    assert v.shape == (P.shape[0], k) and v.dtype == torch.float32 and i.dtype == torch.int32
    assert torch.equal(_bits(v), _bits(v2)) and torch.equal(i, i2)
    sv, si = torch.sort(P.cpu(), dim=-1, descending=True, stable=True)
    assert torch.equal(i.cpu().long(), si[:, :k])
    assert torch.equal(_bits(v.cpu()), _bits(sv[:, :k]))


@pytest.mark.parametrize("B,L,A", SHAPES)
def test_topk_of_go_probs(B, L, A):
    P = _go_probs(B, L, A)
    for k in (1, 5, 32, 64):
        _check_topk(P, min(k, A))
    if A == 8943:       # whether real outputs hold exact fp32 ties near the top (the tie matrices below always do)
        s = torch.sort(P.cpu(), dim=-1, descending=True, stable=True).values[:, :32]
        ties = int((s[:, 1:] == s[:, :-1]).any(-1).sum())
        print(f"top-k B={B} A={A}: rows with an exact tie in the top 32: {ties}")


@pytest.mark.parametrize("shape", [(17, 8943), (3, 70)])
def test_topk_ties(shape):
    torch.manual_seed(sum(shape))
    P = (torch.randint(0, 8, shape, device="cuda") / 8).float()
    for k in (1, 5, 32, 64):
        _check_topk(P, k)


def test_topk_strided_views():
    torch.manual_seed(5)
    big = (torch.randint(0, 64, (17, 9000), device="cuda") / 64).float()
    rows = big[:, 3:8946]                       # row stride 9000, unit column stride, base not 16-B aligned
    assert not rows.is_contiguous()
    _check_topk(rows, 64)
    _check_topk(big[::2, 5:300], 17)            # every other row
    _check_topk(big[:, ::2], 9)                 # column-strided: made contiguous by the wrapper
    _check_topk(big[:, 100:2100], 33)           # 2000 columns: the 64-values-per-lane instantiation


def test_topk_limits_raise_before_any_launch():
    from proteinbert_pytorch_replication_amd.ops import _lib
    from proteinbert_pytorch_replication_amd.ops.infer_heads import TOPK_MAX_COLS, row_topk, topk_supported
    assert topk_supported(8943, 64) and topk_supported(TOPK_MAX_COLS, 1) and topk_supported(5, 5)
    assert not topk_supported(8943, 65) and not topk_supported(8943, 0) and not topk_supported(5, 6)
    assert not topk_supported(TOPK_MAX_COLS + 1, 1)
    calls = []
    real = _lib.call
    _lib.call = lambda *a: calls.append(a)      # any launch attempt would be recorded
    try:
        for A, k in ((8943, 65), (8943, 0), (5, 6), (TOPK_MAX_COLS + 1, 1)):
            with pytest.raises(ValueError, match="outside the kernel's range"):
                row_topk(torch.zeros(2, A, device="cuda"), k)
    finally:
        _lib.call = real
    assert not calls
    _check_topk(torch.rand(2, TOPK_MAX_COLS, device="cuda"), 64)   # the largest supported row


@pytest.mark.parametrize("B,L", [(5, 37), (130, 37)])
def test_masked_mean_pool(B, L):
    from proteinbert_pytorch_replication_amd.ops.infer_heads import masked_mean_pool
    torch.manual_seed(B + L)
    h = torch.randn(B, L, 128, device="cuda").to(torch.bfloat16)
    tokens = torch.randint(1, V, (B, L), device="cuda")
    tokens[torch.rand(B, L, device="cuda") < 0.2] = 0               # pads anywhere
    tokens[0] = 0                                                   # an all-pad row
    tokens[1, : L // 2] = torch.randint(1, V, (L // 2,), device="cuda")
    tokens[1, L // 2:] = 0                                          # a half-padded row
    tokens[2] = torch.randint(1, V, (L,), device="cuda")            # a full row
    out = masked_mean_pool(h, tokens)
    out2 = masked_mean_pool(h, tokens)
    torch.cuda.synchronize()
    assert out.shape == (B, 128) and out.dtype == torch.float32
    assert torch.equal(_bits(out), _bits(out2))
    m = (tokens.cpu() != 0).unsqueeze(-1).to(F64)
    h64 = h.cpu().to(F64)
    cnt = m.sum(1)
    ref = (h64 * m).sum(1) / cnt.clamp(min=1)
    bound = (L + 1) * EPS * (h64.abs() * m).sum(1) / cnt.clamp(min=1)
    got = out.cpu()
    assert int(cnt[0]) == 0 and (got[0] == 0).all() and int(cnt[1]) == L // 2 and int(cnt[2]) == L
    err = (got.to(F64) - ref).abs()
    print(f"pool B={B} L={L}: worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert (err <= bound).all()
