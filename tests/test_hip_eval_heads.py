"""GPU: the gradient-free evaluation heads (ops/eval_heads.py: csrc/evalhead.hip, EPI_GO_EVAL in csrc/gemm.hip)
alone, on random bf16 encoder outputs, against an fp64 CPU reference built from the same bf16 ``h`` / ``g`` and
the bf16-rounded ``Wo`` / ``Wa`` (the kernels read Wo as a bf16 LDS tile and Wa through ``bf16_of``).

Shapes: partial 16 x 32 local tiles, a partial second 128-row GEMM tile, A < 128 and A = 69 * 128 + 111, B above
1024.  Losses within the 1e-3 relative bound of tests/test_hip_heads.py; denominators and histogram totals
exactly; hit counts and histogram edges up to the reference's own near-ties, whose width comes from the error
of an independent fp32 torch evaluation (e_P, e_p) times 16 (``__expf`` and the MFMA accumulation order)."""
import functools
import socket

import pytest
import torch

from proteinbert_pytorch_replication_amd.models import ProteinBERT

pytestmark = pytest.mark.gpu

SHAPES = [(6, 24, 96), (17, 33, 96), (130, 37, 96), (300, 37, 8943), (1030, 9, 96)]
G = 256
F64 = torch.float64


@functools.lru_cache(maxsize=None)
def _case(B, L, A):
    """Inputs on the GPU and the fp64 CPU reference of both heads, computed once per shape and only read."""
    torch.manual_seed(B + L)
    m = ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64, num_heads=4,
                    num_blocks=1, device="cuda", backend="hip")
    h = torch.randn(B, L, 128, device="cuda").to(torch.bfloat16)
    g_bf = torch.randn(B, G, device="cuda").to(torch.bfloat16)
    y_l = torch.randint(0, 26, (B, L), device="cuda")
    x_l = torch.where(torch.rand(B, L, device="cuda") < 0.05, torch.randint(0, 26, (B, L), device="cuda"), y_l)
    w_l = (torch.rand(B, L, device="cuda") < 0.9).float()
    y_g = (torch.rand(B, A, device="cuda") < 0.05).float()
    row = (torch.rand(B, 1, device="cuda") < 0.8).float()
    row[0] = 0
    row[B - 1] = 1
    w_row = row.expand(B, A)                                       # per-row form (stride 0), some zero rows
    w_full = ((torch.rand(B, A, device="cuda") < 0.7).float() * row).contiguous()
    lo, go = m.pretraining_local_output[0], m.pretraining_global_output[0]
    c = dict(m=m, h=h, g_bf=g_bf, y_l=y_l, x_l=x_l, w_l=w_l, y_g=y_g, w_row=w_row, w_full=w_full, lo=lo, go=go)
    # ---- fp64 reference (CPU)
    h64 = h.cpu().to(F64)
    wo = lo.weight.detach().to(torch.bfloat16).cpu()
    bo = lo.bias.detach().cpu()
    Z = h64 @ wo.to(F64).t() + bo.to(F64)
    Z32 = h.cpu().float() @ wo.float().t() + bo                    # the independent fp32 evaluation
    yl, wl = y_l.cpu(), w_l.cpu().to(F64)
    c["counted"] = w_l.cpu() > 0
    c["masked"] = c["counted"] & (x_l.cpu() != yl)
    for name, dim in (("ref", 0), ("paper", -1)):
        P = torch.softmax(Z, dim=dim)
        P32 = torch.softmax(Z32, dim=dim)
        e_P = float(((P32.to(F64) - P).abs() / P).max())
        top = P.topk(2, dim=-1).values
        near = (top[..., 0] - top[..., 1]) / top[..., 0] < 16 * e_P
        py = P.gather(-1, yl.unsqueeze(-1)).squeeze(-1)
        ce = (torch.logsumexp(P, dim=-1) - py) if name == "ref" else -torch.log(py)
        c[name] = dict(e_P=e_P, near=near, hit=P.argmax(-1) == yl, loss=float((ce * wl).mean()))
    wa = go.weight.detach().to(torch.bfloat16).cpu()
    ba = go.bias.detach().cpu()
    z = g_bf.cpu().to(F64) @ wa.to(F64).t() + ba.to(F64)
    p = torch.sigmoid(z)
    p32 = torch.sigmoid(g_bf.cpu().float() @ wa.float().t() + ba)
    c["e_p"] = float(((p32.to(F64) - p).abs() / p).max())
    c["p"] = p
    c["bce"] = -(y_g.cpu().to(F64) * torch.log(p).clamp_min(-100) + (1 - y_g.cpu().to(F64)) *
                 torch.log1p(-p).clamp_min(-100))
    return c


def _check_local(c, ref, lparts, cparts, tag):
    cnt = cparts.sum(0).tolist()
    loss = float(lparts.double().sum())
    counted, masked, near, hit = c["counted"], c["masked"], ref["near"], ref["hit"]
    n, nm = int(counted.sum()), int(masked.sum())
    hits, mhits = int((counted & hit).sum()), int((masked & hit).sum())
    nt, nmt = int((counted & near).sum()), int((masked & near).sum())
    print(f"{tag}: e_P {ref['e_P']:.3e} loss {loss:.6f} ref {ref['loss']:.6f} | counted {cnt[0]} / {n} hits {cnt[1]} / "
          f"{hits} (near-ties {nt}) | masked {cnt[2]} / {nm} hits {cnt[3]} / {mhits} (near-ties {nmt})")
    assert abs(loss - ref["loss"]) < 1e-3 * abs(ref["loss"])
    assert cnt[0] == n and cnt[2] == nm
    assert int(near.sum()) <= 0.01 * near.numel(), "uninformative: too many near-ties in the reference"
    assert abs(cnt[1] - hits) <= nt
    assert abs(cnt[3] - mhits) <= nmt


@pytest.mark.parametrize("B,L,A", SHAPES)
def test_local_head_eval_reference_semantics(B, L, A):
    from proteinbert_pytorch_replication_amd.ops.eval_heads import local_head_eval
    c = _case(B, L, A)
    run = lambda: local_head_eval(c["h"], c["lo"].weight, c["lo"].bias, c["x_l"], c["y_l"], c["w_l"])   # noqa: E731
    lparts, cparts = run()
    l2, c2 = run()
    torch.cuda.synchronize()
    assert cparts.dtype == torch.int32 and cparts.shape[1] == 4
    assert torch.equal(lparts, l2) and torch.equal(cparts, c2)       # bitwise repeatable
    _check_local(c, c["ref"], lparts.cpu(), cparts.cpu().long(), f"ref B={B} L={L}")


@pytest.mark.parametrize("B,L,A", [(17, 33, 96), (130, 37, 96)])
def test_local_head_eval_paper_semantics(B, L, A):
    from proteinbert_pytorch_replication_amd.ops.eval_heads import paper_head_eval
    c = _case(B, L, A)
    run = lambda: paper_head_eval(c["h"], c["lo"].weight, c["lo"].bias, c["x_l"], c["y_l"], c["w_l"])   # noqa: E731
    lparts, cparts = run()
    l2, c2 = run()
    torch.cuda.synchronize()
    assert torch.equal(lparts, l2) and torch.equal(cparts, c2)
    _check_local(c, c["paper"], lparts.cpu(), cparts.cpu().long(), f"paper B={B} L={L}")


@pytest.mark.parametrize("wform", ["row", "full"])
@pytest.mark.parametrize("B,L,A", SHAPES)
def test_go_head_eval(B, L, A, wform):
    from proteinbert_pytorch_replication_amd.ops.eval_heads import go_head_eval
    c = _case(B, L, A)
    w_g = c["w_row"] if wform == "row" else c["w_full"]
    run = lambda: go_head_eval(c["g_bf"], c["go"].weight, c["go"].bias, c["y_g"], w_g)   # noqa: E731
    lparts, hparts = run()
    l2, h2 = run()
    torch.cuda.synchronize()
    assert hparts.shape[1:] == (2, 256) and lparts.numel() == ((B + 127) // 128) * ((A + 127) // 128)
    assert torch.equal(lparts, l2) and torch.equal(hparts, h2)       # bitwise repeatable
    w = w_g.cpu().to(F64)
    ref_loss = float((c["bce"] * w).mean())
    loss = float(lparts.double().sum())
    hist = hparts.cpu().long().sum(0)                                 # [2, 256]
    delta = 16 * c["e_p"] + 2.0 ** -24
    edges = torch.arange(1, 256, dtype=F64) / 256
    sel, pos = w > 0, c["y_g"].cpu() > 0.5
    near_total = 0
    for k, cls in enumerate((sel & pos, sel & ~pos)):
        p = c["p"][cls].sort().values
        assert int(hist[k].sum()) == p.numel()                        # totals exactly
        cum_ref = torch.searchsorted(p, edges)                        # entries below each edge
        cum_got = hist[k].cumsum(0)[:-1]
        near = torch.searchsorted(p, edges + delta, right=True) - torch.searchsorted(p, edges - delta)
        near_total += int(near.sum())
        bad = (cum_got - cum_ref).abs() > near
        assert not bad.any(), (k, edges[bad][:4], cum_got[bad][:4], cum_ref[bad][:4])
    share = near_total / max(1, int(sel.sum()))
    print(f"GO B={B} A={A} {wform}: e_p {c['e_p']:.3e} delta {delta:.3e} loss {loss:.6f} ref {ref_loss:.6f} "
          f"pos {int(hist[0].sum())} neg {int(hist[1].sum())} within-delta share {share:.2e}")
    assert share <= 0.02, "uninformative: too many entries at the bin edges"
    assert abs(loss - ref_loss) < 1e-3 * abs(ref_loss)


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_eval_heads_fold_accumulates(semantics):
    """eval_heads (both heads + the fold) twice into one accumulator: exactly twice the integer partial sums,
    the fp64 loss sums, int64 / fp64 storage, batch and sequence counters."""
    from proteinbert_pytorch_replication_amd.ops import eval_heads as eh
    B, L, A = 130, 37, 96
    c = _case(B, L, A)
    m = c["m"]
    prev = m.semantics
    m.semantics = semantics                      # the heads' parameters are the same for both semantics
    try:
        acc = eh.EvalAccumulator("cuda")
        Y, W = {"local": c["y_l"], "global": c["y_g"]}, {"local": c["w_l"], "global": c["w_row"]}
        for _ in range(2):
            eh.eval_heads(m, c["h"], None, c["g_bf"], c["x_l"], Y, W, acc)
    finally:
        m.semantics = prev
    local = eh.paper_head_eval if semantics == "paper" else eh.local_head_eval
    ll, lc = local(c["h"], c["lo"].weight, c["lo"].bias, c["x_l"], c["y_l"], c["w_l"])
    gl, gh = eh.go_head_eval(c["g_bf"], c["go"].weight, c["go"].bias, c["y_g"], c["w_row"])
    torch.cuda.synchronize()
    assert acc.counts.dtype == torch.int64 and acc.loss.dtype == torch.float64
    cnt = acc.counts.cpu()
    assert cnt[:2].tolist() == [2, 2 * B] and cnt[6:8].tolist() == [0, 0]
    assert cnt[2:6].tolist() == (2 * lc.long().sum(0)).tolist()
    assert torch.equal(cnt[8:], 2 * gh.long().sum(0).reshape(-1).cpu())
    assert torch.equal(acc.hist_pos.cpu(), cnt[8:264]) and torch.equal(acc.hist_neg.cpu(), cnt[264:])
    want = 2 * torch.stack([ll.double().sum(), gl.double().sum()]).cpu()
    assert ((acc.loss.cpu() - want).abs() <= 1e-12 * want.abs()).all()


def test_local_head_eval_shared_batch_softmax_forced():
    """batch_softmax forced active on a 1-rank group: stage A leaves the raw (M, S) and the statistics go
    through the cross-rank merge; with one rank the result is the plain one (the merge's exp(M - M) = 1 is exact;
    only its 1 / S runs in torch instead of in the fold kernel)."""
    import datetime
    import torch.distributed as dist
    from proteinbert_pytorch_replication_amd.ops.eval_heads import local_head_eval
    from proteinbert_pytorch_replication_amd.parallel import batch_softmax
    c = _case(130, 37, 96)
    run = lambda: local_head_eval(c["h"], c["lo"].weight, c["lo"].bias, c["x_l"], c["y_l"], c["w_l"])   # noqa: E731
    l0, c0 = run()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            timeout=datetime.timedelta(seconds=60))
    try:
        batch_softmax.enable(force=True)
        assert batch_softmax.active()
        l1, c1 = run()
        torch.cuda.synchronize()
    finally:
        batch_softmax.disable()
        dist.destroy_process_group()
    a, b = c0.long().sum(0).tolist(), c1.long().sum(0).tolist()
    ref = c["ref"]
    assert a[0] == b[0] and a[2] == b[2]
    assert abs(a[1] - b[1]) <= int((c["counted"] & ref["near"]).sum())
    assert abs(a[3] - b[3]) <= int((c["masked"] & ref["near"]).sum())
    s0, s1 = float(l0.double().sum()), float(l1.double().sum())
    assert abs(s0 - s1) <= 1e-6 * abs(s0)
    _check_local(c, ref, l1.cpu(), c1.cpu().long(), "ref shared-softmax B=130 L=37")
