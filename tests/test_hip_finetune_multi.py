"""``hidden="all"`` fine-tuning head on the GPU: the multi-source token-head kernels of csrc/finetune.hip
(``pbx_token_head_multi_fwd`` / ``pbx_token_head_multi_wgrad``) against fp64, and the whole model on the
fused encoder."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

CH = 128
# (B, L, nb, K, gterm): M = 37 fills part of one 256-row workgroup; M = 500 puts the sample boundary 2|3 (row 300)
# inside the second tile, so the gterm row changes within a tile; M = 3000 is 12 tiles, the last one partial.
# Every nb in {1, 2, 6, 8}, every K in {1, 8, 13, 16}, gterm null and given.
CASES = [(1, 37, 1, 1, False), (1, 37, 2, 13, True), (5, 100, 6, 8, True), (5, 100, 8, 16, False),
         (5, 100, 1, 13, True), (3, 1000, 6, 8, True), (3, 1000, 2, 16, True), (3, 1000, 8, 1, False)]
U24 = 2.0 ** -24


def _lib():
    from proteinbert_pytorch_replication_amd.ops import _lib
    return _lib


def _srcs(rows):
    return (ctypes.c_void_p * len(rows))(*[r.data_ptr() for r in rows])


def _multi_fwd(rows, W, b, gt, out, M, K, L):
    lib = _lib()
    lib.call("pbx_token_head_multi_fwd", _srcs(rows), len(rows), W.data_ptr(), b.data_ptr(), lib.ptr(gt),
             out.data_ptr(), M, K, L, lib.stream_ptr(out.device))
    return out


@functools.lru_cache(maxsize=None)
def _case(B, L, nb, K, with_g):
    """Seeded inputs and the fp64 evaluation of the definition on the same bf16 rows and fp32 weights (computed
    once per case; the tests only read it)."""
    gen = torch.Generator(device="cuda").manual_seed(1000 * nb + 10 * K + B)
    hs = [torch.randn(B, L, CH, device="cuda", generator=gen).to(torch.bfloat16) for _ in range(nb)]
    W = torch.randn(K, nb * CH, device="cuda", generator=gen) * 0.1
    b = torch.randn(K, device="cuda", generator=gen)
    gt = torch.randn(B, K, device="cuda", generator=gen) if with_g else None
    dl = torch.randn(B, L, K, device="cuda", generator=gen)
    cat = torch.cat([h.double() for h in hs], -1)                               # [B, L, nb*128]
    ref = cat @ W.double().T + b.double()
    mag = cat.abs() @ W.double().abs().T + b.double().abs()
    if with_g:
        ref = ref + gt.double().unsqueeze(1)
        mag = mag + gt.double().abs().unsqueeze(1)
    g64 = dl.double().reshape(B * L, K)
    grads = {"dW": g64.T @ cat.reshape(B * L, -1), "db": g64.sum(0), "dh": g64 @ W.double(),
             "dgt": dl.double().sum(1)}
    return {"hs": hs, "W": W, "b": b, "gt": gt, "dl": dl, "ref": ref, "mag": mag, "grads": grads}


def _run_fn(c, grad=True):
    from proteinbert_pytorch_replication_amd.ops.finetune_head import MultiTokenHeadFn, supported_multi
    hs = [h.clone().requires_grad_(grad) for h in c["hs"]]
    W, b = c["W"].clone().requires_grad_(grad), c["b"].clone().requires_grad_(grad)
    gt = None if c["gt"] is None else c["gt"].clone().requires_grad_(grad)
    assert supported_multi(hs, W.shape[0])
    out = MultiTokenHeadFn.apply(*hs, W, b, gt)
    if grad:
        (out * c["dl"]).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), hs, W, b, gt


@pytest.mark.parametrize("B,L,nb,K,with_g", CASES)
def test_multi_forward_within_fp32_running_error_bound(B, L, nb, K, with_g):
    c = _case(B, L, nb, K, with_g)
    out, *_ = _run_fn(c, grad=False)
    assert out.shape == (B, L, K) and out.dtype == torch.float32
    err = (out.double() - c["ref"]).abs()
    bound = (nb * CH + 2) * U24 * c["mag"]          # fp32 running-error bound of a sum of nb*128 + 2 terms
    worst = (err / bound).max().item()
    print(f"multi fwd B={B} L={L} nb={nb} K={K} gterm={with_g}: max err/bound = {worst:.4f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("B,L,K", [(1, 37, 1), (5, 100, 13), (3, 1000, 8), (3, 1000, 16)])
def test_single_source_is_bitwise_token_head_fwd(B, L, K):
    lib = _lib()
    c = _case(B, L, 1, K, False)
    M = B * L
    rows = c["hs"][0].view(M, CH)
    out = _multi_fwd([rows], c["W"], c["b"], None, torch.empty((M, K), device="cuda"), M, K, L)
    one = torch.empty((M, K), device="cuda")
    lib.call("pbx_token_head_fwd", rows.data_ptr(), c["W"].data_ptr(), c["b"].data_ptr(), one.data_ptr(), M, K,
             lib.stream_ptr(one.device))
    torch.cuda.synchronize()
    assert torch.equal(out, one)                    # the same FMA order


@pytest.mark.parametrize("B,L,nb,K,with_g", CASES)
def test_multi_backward_matches_fp64(B, L, nb, K, with_g):
    c = _case(B, L, nb, K, with_g)
    _, hs, W, b, gt = _run_fn(c)
    rel = lambda a, r: ((a.double() - r).norm() / r.norm()).item()  # noqa: E731
    g = c["grads"]
    figs = {"dW": rel(W.grad, g["dW"]), "db": rel(b.grad, g["db"])}
    for i, h in enumerate(hs):
        figs[f"dh{i}"] = rel(h.grad.view(B * L, CH), g["dh"][:, i * CH:(i + 1) * CH])
    if with_g:
        figs["dgt"] = rel(gt.grad, g["dgt"])
    print(f"multi bwd B={B} L={L} nb={nb} K={K}: " + " ".join(f"{k}={v:.2e}" for k, v in figs.items()))
    assert figs["dW"] < 1e-5 and figs["db"] < 1e-5      # tests/test_finetune.py's bounds
    assert all(figs[f"dh{i}"] < 5e-3 for i in range(nb))
    assert all(h.grad.dtype == torch.bfloat16 for h in hs)
    if with_g:
        assert figs["dgt"] < 1e-5


@pytest.mark.parametrize("B,L,nb,K,with_g", [CASES[2], CASES[3], CASES[5]])
def test_multi_head_repeats_bitwise(B, L, nb, K, with_g):
    c = _case(B, L, nb, K, with_g)
    o1, _, W1, *_ = _run_fn(c)
    o2, _, W2, *_ = _run_fn(c)
    assert torch.equal(o1, o2) and torch.equal(W1.grad, W2.grad)


@pytest.mark.parametrize("B,L,nb,K,with_g", [CASES[1], CASES[2], CASES[7]])
def test_tail_rows_untouched_and_offset_sources(B, L, nb, K, with_g):
    """Rows >= M of the output stay as allocated; a source that is a row-offset view into a larger allocation
    gives the result of a compact copy."""
    lib = _lib()
    c = _case(B, L, nb, K, with_g)
    M, pad, SENT = B * L, 300, -12345.5
    compact = [h.view(M, CH) for h in c["hs"]]
    want = _multi_fwd(compact, c["W"], c["b"], c["gt"], torch.empty((M, K), device="cuda"), M, K, L)
    views = []
    for i, h in enumerate(compact):
        big = torch.full((M + 2 * pad, CH), float("nan"), device="cuda", dtype=torch.bfloat16)
        off = 1 + 7 * i                                # any row offset keeps the 256-B rows 16-byte aligned
        big[off:off + M] = h
        views.append(big[off:off + M])
    out = torch.full((M + pad, K), SENT, device="cuda")
    _multi_fwd(views, c["W"], c["b"], c["gt"], out, M, K, L)
    # weight gradient from the offset views, into a slab with sentinel rows behind its P partial rows
    g = c["dl"].reshape(M, K).contiguous()
    P = 7
    slab = torch.full((P + 2, K, nb * CH), SENT, device="cuda")
    lib.call("pbx_token_head_multi_wgrad", _srcs(views), nb, g.data_ptr(), slab.data_ptr(), M, K, P,
             lib.stream_ptr(g.device))
    slab_c = torch.empty((P, K, nb * CH), device="cuda")
    lib.call("pbx_token_head_multi_wgrad", _srcs(compact), nb, g.data_ptr(), slab_c.data_ptr(), M, K, P,
             lib.stream_ptr(g.device))
    torch.cuda.synchronize()
    assert torch.equal(out[:M], want)
    assert bool((out[M:] == SENT).all())
    assert torch.equal(slab[:P], slab_c) and bool((slab[P:] == SENT).all())
    dW = slab_c.double().sum(0)
    assert ((dW - c["grads"]["dW"]).norm() / c["grads"]["dW"].norm()).item() < 1e-5
    assert {"pbx_token_head_multi_fwd", "pbx_token_head_multi_wgrad"} <= set(lib._FN)     # the session's report


def test_launchers_refuse_bad_arguments():
    lib = _lib()
    c = _case(1, 37, 1, 1, False)
    rows = c["hs"][0].view(37, CH)
    out = torch.empty((37, 1), device="cuda")
    for nb, K in [(0, 1), (9, 1), (1, 17), (1, 0)]:
        with pytest.raises(lib.HipError):
            lib.call("pbx_token_head_multi_fwd", _srcs([rows] * max(1, nb)), nb, c["W"].data_ptr(), c["b"].data_ptr(),
                     None, out.data_ptr(), 37, K, 37, lib.stream_ptr(out.device))


# ---- the whole model on the fused encoder ------------------------------------------------------------------------
def _hip_encoder(semantics="reference", seed=0, L=128):
    from proteinbert_pytorch_replication_amd.models import ProteinBERT
    torch.manual_seed(seed)
    return ProteinBERT(sequences_length=L, num_annotations=256, local_dim=128, global_dim=512, key_dim=64,
                       num_heads=4, num_blocks=2, device="cuda", backend="hip", semantics=semantics)


def _batch(L=128, K=8):
    from proteinbert_pytorch_replication_amd.data.synthetic import SyntheticSecondaryStructure
    ds = SyntheticSecondaryStructure(16, L, n_classes=K)
    return ds.tokens.cuda(), ds.labels.cuda()


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_all_block_head_on_fused_encoder(semantics):
    from proteinbert_pytorch_replication_amd.models import ProteinBERTForTokenClassification
    from proteinbert_pytorch_replication_amd.models.finetune import _split_inputs
    from proteinbert_pytorch_replication_amd.ops.fused_model import fused_encode
    enc = _hip_encoder(semantics)
    K, nb = 8, 2
    model = ProteinBERTForTokenClassification(enc, n_classes=K, hidden="all")
    X, _ = _batch()
    out = model(X)                                               # [B, K, L]
    assert out.shape == (16, K, 128)
    # the head alone: the fused encoder's own tapped states through the definition in torch
    hs, gs = [], []
    tok, ann = _split_inputs(enc, X)
    with torch.no_grad():
        fused_encode(enc, tok, ann, tap=lambda i, h, g: (hs.append(h), gs.append(g)))
        W, b = model.head.weight, model.head.bias
        gterm = model.global_head(torch.cat([g.float() for g in gs], -1))
        cat = torch.cat([h.float() for h in hs], -1)
        ref32 = torch.nn.functional.linear(cat, W, b) + gterm.unsqueeze(1)
        ref64 = cat.double() @ W.double().T + b.double() + gterm.double().unsqueeze(1)
        mag = cat.double().abs() @ W.double().abs().T + b.double().abs() + gterm.double().abs().unsqueeze(1)
    assert len(hs) == nb and hs[0].dtype == torch.bfloat16
    bound = (nb * CH + 2) * U24 * mag
    got = out.detach().permute(0, 2, 1).double()
    e32, e64 = (got - ref32.double()).abs(), (got - ref64).abs()
    print(f"{semantics}: head vs fp32 definition max err/bound = {(e32 / bound).max().item():.4f}, "
          f"vs fp64 = {(e64 / bound).max().item():.4f}")
    assert bool((e32 <= bound).all()) and bool((e64 <= bound).all())
    # the whole model against the torch backend, at test_hip_encoder_finetune_matches_torch_encoder's tolerance
    enc.backend = "torch"
    out_ref = model(X)
    enc.backend = "hip"
    torch.testing.assert_close(out, out_ref, rtol=0.05, atol=0.05)


def test_all_block_head_unfrozen_reaches_every_block():
    from proteinbert_pytorch_replication_amd.models import ProteinBERTForTokenClassification
    from proteinbert_pytorch_replication_amd.train.finetune import train_step
    from proteinbert_pytorch_replication_amd.train.optim import FusedAdam
    X, y = _batch()
    C, G = 128, 512
    grads = {}
    torch.manual_seed(3)
    w_last, gw_last = torch.randn(8, C, device="cuda") * 0.1, torch.randn(8, G, device="cuda") * 0.05
    w_first = torch.randn(8, C, device="cuda") * 0.1
    for hidden in ("last", "all"):
        enc = _hip_encoder(seed=0)
        m = ProteinBERTForTokenClassification(enc, n_classes=8, freeze_encoder=False, hidden=hidden)
        with torch.no_grad():
            # the same last-block head in both runs; "all" adds only block 0's local states (its global slice is
            # zero), so block 0's gradients differ exactly when the head's dh_0 arrives
            m.head.bias.zero_()
            if hidden == "last":
                m.head.weight.copy_(w_last)
                m.global_head.weight.copy_(gw_last)
            else:
                m.head.weight.copy_(torch.cat([w_first, w_last], 1))
                m.global_head.weight.copy_(torch.cat([torch.zeros_like(gw_last), gw_last], 1))
        opt = FusedAdam(m.parameters(), lr=1e-4)
        tl, _ = train_step(m, [(X, y)], torch.nn.CrossEntropyLoss(ignore_index=-100), opt, {}, True, 1.0, "cuda")
        assert tl == tl and abs(tl) != float("inf")
        blocks = enc.proteinBERT_blocks
        grads[hidden] = [blocks[i].local_narrow_conv_layer[0].weight.grad.detach().clone() for i in (0, -1)]
        assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads[hidden])
    d = (grads["all"][0] - grads["last"][0]).norm() / grads["last"][0].norm()
    print(f"block-0 conv gradient, all vs last: relative difference {d.item():.3e}")
    assert not torch.equal(grads["all"][0], grads["last"][0])


def test_hidden_last_on_hip_is_bitwise_the_class_without_the_keyword():
    from proteinbert_pytorch_replication_amd.models import ProteinBERTForTokenClassification
    X, _ = _batch()
    outs = []
    for kw in ({}, {"hidden": "last"}):
        enc = _hip_encoder(seed=0)
        torch.manual_seed(7)
        outs.append(ProteinBERTForTokenClassification(enc, n_classes=8, **kw)(X))
    assert torch.equal(outs[0], outs[1])
