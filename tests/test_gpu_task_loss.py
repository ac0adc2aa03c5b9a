"""GPU: the fused residue training loss through a whole model (``ProteinBERTForTokenClassification.loss`` under
``train.finetune.train_step``) in both semantics: 2 blocks, L = 128, B = 8, K = 3, ``hidden`` last and all, class
weights and label smoothing.

Two batches are trained with the fused path (``ops.finetune_head.LOSS_FUSED``) and, from the same initial state,
with it disabled (``loss_fn(model(X), y)``, the torch loss ops and their backward).

Loss per batch: each path against the fp64 loss of that model's own ``forward`` logits (bit for bit the logits the
loss kernel holds), within the kernel test's budget: ``sum_rows (16 e_L + 2^-24 (1 + loss_row)) + n 2^-24
sum |loss_row|`` over the sum of the row weights, plus the fp32 summation of those weights and the rounding of the
quotient (``(n + 1) 2^-24`` relative), ``e_L`` being the worst per-row error of the fp32 torch evaluation.
Accuracy per batch: the fp64 calls, except on rows whose top two fp64 probabilities lie within twice the probability
bound of tests/test_hip_task_calls.py (``16 e_P P + 2^-24``), where either call is admissible.

Head parameters after the two Adam steps: fused against unfused within 16 times the difference ``d`` measured between
two fp32 torch evaluations of the same two steps on the same (frozen) encoder rows that differ only in summation
order (the rows of a batch in natural and in a fixed shuffled order: the loss sum and the 1024-long reductions of
``dW``, ``db`` and ``dgt`` then add the same numbers in another order), plus the fp32 rounding of the parameter.  Adam
divides the gradient by its own magnitude, so a parameter moves by the relative, not the absolute, gradient error;
``d`` is taken per parameter tensor as the largest element difference, which the smallest gradients dominate in both
pairs, and 16 is the width this project grants a kernel against an fp32 torch evaluation."""
import functools

import pytest
import torch
import torch.nn.functional as F

from proteinbert_pytorch_replication_amd.models import ProteinBERT, ProteinBERTForTokenClassification

pytestmark = pytest.mark.gpu

L, A, G, BLOCKS, B, K = 128, 256, 256, 2, 8, 3
F64 = torch.float64
EPS = 2.0 ** -24
CW, SMOOTH, LR = [0.4, 1.0, 1.7], 0.1, 1e-2


def _model(semantics, hidden, freeze=True):
    torch.manual_seed(0)
    # the paper-semantics HIP attention core is built for value_dim = G / heads = 128
    enc = ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64,
                      num_heads=4 if semantics == "reference" else 2, num_blocks=BLOCKS, device="cuda",
                      backend="hip", semantics=semantics)
    torch.manual_seed(21)
    return ProteinBERTForTokenClassification(enc, n_classes=K, freeze_encoder=freeze, hidden=hidden)


@functools.lru_cache(maxsize=None)
def _batches():
    gen = torch.Generator().manual_seed(9)
    out = []
    for _ in range(2):
        lens = torch.randint(20, L - 1, (B,), generator=gen)
        tok = torch.randint(4, 26, (B, L), generator=gen)
        pos = torch.arange(L).unsqueeze(0)
        tok[:, 0] = 1
        tok = torch.where(pos == lens[:, None] + 1, torch.full_like(tok, 2), tok)
        tok = torch.where(pos > lens[:, None] + 1, torch.zeros_like(tok), tok)
        y = torch.randint(0, K, (B, L), generator=gen)
        y[torch.rand(B, L, generator=gen) < 0.2] = -100
        y[tok < 3] = -100
        out.append((tok.cuda(), y.cuda()))
    return out


def _reference(logits, y, cw):
    """fp64 loss, its budget and the admissible accuracy range, from fp32 logits ``[B, K, L]`` (exact inputs)."""
    z32 = logits.detach().float().permute(0, 2, 1).reshape(-1, K).cpu()
    z, yf, w = z32.to(F64), y.view(-1).cpu(), cw.to(F64)
    live = yf >= 0
    ys = yf.clamp_min(0)
    lp = torch.log_softmax(z, -1)
    rows = ((1 - SMOOTH) * w[ys] * -(lp.gather(-1, ys[:, None])[:, 0]) + (SMOOTH / K) * (w * -lp).sum(-1))[live]
    rows32 = F.cross_entropy(z32, yf, weight=cw, ignore_index=-100, label_smoothing=SMOOTH, reduction="none")[live]
    e_L = float((rows32.to(F64) - rows).abs().max())
    n, sw = int(live.sum()), float(w[ys][live].sum())
    budget = float((16 * e_L + EPS * (1 + rows)).sum() + n * EPS * rows.abs().sum())
    loss = float(rows.sum()) / sw
    tol = budget / sw + (n + 1) * EPS * loss
    P = lp.exp()
    e_P = float(((torch.softmax(z32, -1).to(F64) - P).abs() / P).max())
    top = P.sort(-1, descending=True).values
    near = live & ((top[:, 0] - top[:, 1]) <= 2 * (16 * e_P * top[:, 0] + EPS))
    hits = int(((P.argmax(-1) == yf) & live & ~near).sum())
    return loss, tol, hits / n, (hits + int(near.sum())) / n


def _train(semantics, hidden, fused):
    """Two ``train_step`` calls of one batch each: per-batch (loss, accuracy, reference), the head parameters after,
    and the launchers that ran during the steps."""
    from proteinbert_pytorch_replication_amd.ops import _lib, finetune_head
    from proteinbert_pytorch_replication_amd.train.finetune import token_accuracy, train_step
    from proteinbert_pytorch_replication_amd.train.task_loss import ResidueTaskLoss
    model = _model(semantics, hidden)
    loss_fn = ResidueTaskLoss(CW, SMOOTH)
    heads = {k: p for k, p in model.named_parameters() if p.requires_grad}
    assert all(not k.startswith("encoder.") for k in heads)
    opt = torch.optim.Adam(heads.values(), lr=LR)
    enc_before = [p.detach().clone() for p in model.encoder.parameters()]
    names, steps = [], []
    real = _lib.call
    was = finetune_head.LOSS_FUSED
    finetune_head.LOSS_FUSED = fused
    try:
        for X, y in _batches():
            with torch.no_grad():
                ref = _reference(model.train()(X), y, torch.tensor(CW))
            _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
            try:
                loss, met = train_step(model, [(X, y)], loss_fn, opt, {"accuracy": token_accuracy()}, device="cuda")
            finally:
                _lib.call = real
            steps.append((loss, met["accuracy"], ref))
    finally:
        finetune_head.LOSS_FUSED = was
    assert model.training and model.head.training and not model.encoder.training
    assert not any(m.training for m in model.encoder.modules())
    assert all(torch.equal(a, b) for a, b in zip(enc_before, model.encoder.parameters()))
    assert all(p.grad is None for p in model.encoder.parameters())
    return steps, {k: p.detach().cpu().clone() for k, p in heads.items()}, names


def _torch_steps(semantics, hidden, shuffled):
    """The same two Adam steps by the definition in fp32 torch on the frozen encoder's rows; ``shuffled``: every
    batch's rows in a fixed random order (only the summation order changes)."""
    model = _model(semantics, hidden)
    heads = {k: p for k, p in model.named_parameters() if p.requires_grad}
    opt = torch.optim.Adam(heads.values(), lr=LR)
    cw = torch.tensor(CW, device="cuda")
    gen = torch.Generator().manual_seed(3)
    for X, y in _batches():
        if hidden == "all":
            hs, gs = model._encode_all(X)
            gin = torch.cat([g.float() for g in gs], dim=-1)
        else:
            h, g = model._encode(X)
            hs, gin = [h], g.float()
        feats = torch.cat([h.float() for h in hs], dim=-1).view(B * L, -1)
        yf = y.view(-1)
        sample = torch.arange(B * L, device="cuda") // L
        if shuffled:
            perm = torch.randperm(B * L, generator=gen).cuda()
            feats, yf, sample = feats[perm], yf[perm], sample[perm]
        z = F.linear(feats, model.head.weight, model.head.bias) + model.global_head(gin)[sample]
        loss = F.cross_entropy(z, yf, weight=cw, ignore_index=-100, label_smoothing=SMOOTH)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(heads.values()), 1)
        opt.step()
    return {k: p.detach().cpu().clone() for k, p in heads.items()}


@pytest.mark.parametrize("semantics", ["reference", "paper"])
@pytest.mark.parametrize("hidden", ["last", "all"])
def test_fused_steps_match_the_unfused_steps(semantics, hidden):
    fused, pf, names_f = _train(semantics, hidden, True)
    plain, pu, names_u = _train(semantics, hidden, False)
    # the fused steps run the new launchers and never the logit kernels; the unfused steps the reverse
    wgrad = "pbx_token_head_wgrad" if hidden == "last" else "pbx_token_head_multi_wgrad"
    assert {"pbx_token_head_loss", "pbx_token_head_loss_fold", wgrad, "pbx_colsum_add"} <= set(names_f)
    assert not {"pbx_token_head_fwd", "pbx_token_head_multi_fwd"} & set(names_f)
    assert names_f.count("pbx_token_head_loss") == 2 and names_f.count("pbx_token_head_loss_fold") == 2
    assert not {"pbx_token_head_loss", "pbx_token_head_loss_fold"} & set(names_u)
    assert ("pbx_token_head_fwd" if hidden == "last" else "pbx_token_head_multi_fwd") in names_u
    for i, ((lf, af, rf), (lu, au, ru)) in enumerate(zip(fused, plain)):
        for tag, l, a, (ref, tol, lo, hi) in (("fused", lf, af, rf), ("unfused", lu, au, ru)):
            print(f"{semantics} {hidden} batch {i} {tag}: loss {l:.7f} ref {ref:.7f} err / tol "
                  f"{abs(l - ref) / tol:.4f}; accuracy {a:.5f} in [{lo:.5f}, {hi:.5f}]")
            assert abs(l - ref) <= tol, (tag, i, l, ref, tol)
            assert lo - EPS <= a <= hi + EPS, (tag, i, a, lo, hi)
        if i == 0:                                  # the same parameters: the same logits, so the same reference
            assert abs(rf[0] - ru[0]) <= EPS * rf[0]
    pa, pb = _torch_steps(semantics, hidden, False), _torch_steps(semantics, hidden, True)
    assert set(pf) == set(pu) == set(pa) == {"head.weight", "head.bias", "global_head.weight"}
    for k in pf:
        d = float((pa[k] - pb[k]).abs().max())
        bound = 16 * d + EPS * float(pu[k].abs().max())
        err = float((pf[k] - pu[k]).abs().max())
        print(f"{semantics} {hidden} {k}: |fused - unfused| {err:.3e}, torch order difference d {d:.3e}, "
              f"err / bound {err / bound:.4f}; |fused - torch| {float((pf[k] - pa[k]).abs().max()):.3e}")
        assert err <= bound, (k, err, bound)
        assert float((pf[k] - pa[k]).abs().max()) <= 0.1 * LR             # and both moved as the definition does


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_an_unfrozen_step_reaches_the_encoder(semantics):
    from proteinbert_pytorch_replication_amd.ops import _lib
    from proteinbert_pytorch_replication_amd.train.task_loss import ResidueTaskLoss
    model = _model(semantics, "all", freeze=False).train()
    modes = [(m, m.training) for m in model.modules()]
    loss_fn = ResidueTaskLoss(CW, SMOOTH)
    X, y = _batches()[0]
    names = []
    real = _lib.call
    _lib.call = lambda name, *a: (names.append(name), real(name, *a))[1]
    try:
        loss, acc = model.loss(X, y, loss_fn)
        loss.backward()
    finally:
        _lib.call = real
    assert "pbx_token_head_loss" in names and "pbx_token_head_multi_fwd" not in names
    assert all(m.training == t for m, t in modes)
    assert torch.isfinite(loss).item() and 0.0 <= float(acc) <= 1.0
    # the pretraining output layers take no part in a residue head: every other encoder parameter has a gradient
    named = [(k, p) for k, p in model.encoder.named_parameters() if p.requires_grad]
    grads = {k: p.grad for k, p in named if p.grad is not None}
    assert len(grads) >= len(named) // 2 and all(torch.isfinite(g).all() for g in grads.values())
    moved = [k for k, g in grads.items() if g.abs().sum() > 0]
    assert len(moved) >= len(grads) // 2 and any("proteinBERT_blocks.0." in k for k in moved)
    cnt = loss_fn.counter("cuda").tolist()
    assert cnt[0] == int((y >= 0).sum()) and cnt[2] == 0 and cnt[1] == round(float(acc) * cnt[0])


def test_labels_outside_the_classes_raise_from_the_fused_step():
    from proteinbert_pytorch_replication_amd.train.finetune import token_accuracy, train_step
    from proteinbert_pytorch_replication_amd.train.task_loss import ResidueTaskLoss
    model = _model("reference", "last")
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=LR)
    loss_fn = ResidueTaskLoss(CW, SMOOTH)
    (X0, y0), (X1, y1) = _batches()
    y0, y1 = y0.clone(), y1.clone()
    y0[2, 5], y0[7, 9], y1[0, 3] = K, 10 ** 6, K + 1
    with pytest.raises(ValueError, match=r"^3 training labels"):
        train_step(model, [(X0, y0), (X1, y1)], loss_fn, opt, {"accuracy": token_accuracy()}, device="cuda")
    # the counter is per epoch: a clean epoch after it passes, on the same loss object
    loss, met = train_step(model, _batches(), loss_fn, opt, {"accuracy": token_accuracy()}, device="cuda")
    assert loss == loss and 0.0 <= met["accuracy"] <= 1.0
    assert loss_fn.counter("cuda") is loss_fn.counter(torch.device("cuda", torch.cuda.current_device()))
