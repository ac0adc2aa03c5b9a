"""GPU: ``train.evaluate_finetune.evaluate_finetune`` on the HIP backend for a whole model in both semantics: the
model of tests/test_gpu_predict_tasks.py (L = 128, A = 256, G = 256, 2 blocks, 19 sequences of mixed lengths in
batches of 8, 8 and 3) with an 8-class ``hidden="last"`` residue head, a 3-class ``hidden="all"`` residue head, a
4-class and a 2-class per-protein head and a regression head.

Residue heads: the confusion matrix equals, exactly, the one built from ``Predictor(...).predict`` labels and ``y``
over the positions with ``y >= 0`` (the two kernels hold identical logits and share the calling rule).  The loss
is compared with ``F.cross_entropy`` on the model's own ``forward`` logits, which are bit for bit the logits the
evaluation kernel holds: per row both sides carry the error of K exponentials (16 ulps granted, the project's
width for ``__expf``), a sum of K terms and a logarithm, ``(18 + K) 2^-24 + 2^-24 ce`` each, and an fp32 sum of n
rows adds ``n 2^-24 sum ce`` on either side.

Per-protein and regression heads: against the head evaluated in fp64 on the ``global`` / ``hidden_global`` states
``Predictor`` returns; a logit of n terms carries at most the fp32 running error d = (n + 2) 2^-24 (|x| . |w| + |b|)
(tests/test_gpu_predict_tasks.py), so a sequence whose top two fp64 logits lie within 2 d is labelled -1 (ignored)
and the remaining calls are exact."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from proteinbert_pytorch_replication_amd import Predictor
from proteinbert_pytorch_replication_amd.models import (ProteinBERT, ProteinBERTForSequenceClassification,
                                                        ProteinBERTForTokenClassification)

pytestmark = pytest.mark.gpu

L, A, G, BLOCKS, N, BS = 128, 256, 256, 2, 19, 8
F64 = torch.float64
EPS = 2.0 ** -24


def _model(semantics, seed=0):
    torch.manual_seed(seed)
    # the paper-semantics HIP attention core is built for value_dim = G / heads = 128
    return ProteinBERT(sequences_length=L, num_annotations=A, local_dim=128, global_dim=G, key_dim=64,
                       num_heads=4 if semantics == "reference" else 2, num_blocks=BLOCKS, device="cuda",
                       backend="hip", semantics=semantics)


def _heads(m):
    torch.manual_seed(21)
    return {"ss8": ProteinBERTForTokenClassification(m, n_classes=8, freeze_encoder=False, hidden="last"),
            "ss3": ProteinBERTForTokenClassification(m, n_classes=3, freeze_encoder=False, hidden="all"),
            "loc": ProteinBERTForSequenceClassification(m, n_classes=4, freeze_encoder=False, hidden="all"),
            "bin": ProteinBERTForSequenceClassification(m, n_classes=2, freeze_encoder=False),
            "stab": ProteinBERTForSequenceClassification(m, n_classes=1, freeze_encoder=False)}


def _sequences():
    rng = np.random.default_rng(7)
    lens = [1, L - 2] + [int(v) for v in rng.integers(5, L - 1, N - 2)]
    return ["".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), n)) for n in lens]


def _batches(tokens, y):
    return [(tokens[s:s + BS], y[s:s + BS]) for s in range(0, N, BS)]


@functools.lru_cache(maxsize=None)
def _setup(semantics):
    m = _model(semantics)
    heads = _heads(m)
    pred = Predictor(m, batch_size=BS, heads={k: heads[k] for k in ("ss8", "ss3")})
    seqs = _sequences()
    tokens = pred.tokenize(seqs)
    out = pred.predict(seqs, outputs=("global", "hidden_states", "task:ss8", "task:ss3"))
    gen = torch.Generator().manual_seed(5)
    ys = {}
    for name, K in (("ss8", 8), ("ss3", 3)):
        y = torch.randint(0, K, (N, L), generator=gen)
        y[torch.rand(N, L, generator=gen) < 0.25] = -100
        y[tokens < 3] = -100                          # <pad>, <sos>, <eos>: what cli finetune labels -100
        ys[name] = y
    return dict(m=m, heads=heads, tokens=tokens, out=out, ys=ys)


def _logits64(head, x):
    W, b = head.head.weight.detach().cpu().to(F64), head.head.bias.detach().cpu().to(F64)
    z = x.to(F64) @ W.T + b
    d = (x.shape[1] + 2) * EPS * (x.to(F64).abs() @ W.abs().T + b.abs())
    return z, d


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_residue_heads_match_predictor_and_forward(semantics):
    from proteinbert_pytorch_replication_amd.ops import _lib, fused_model
    from proteinbert_pytorch_replication_amd.train.evaluate_finetune import evaluate_finetune
    r = _setup(semantics)
    m, heads, tokens = r["m"], r["heads"], r["tokens"]
    for name, K in (("ss8", 8), ("ss3", 3)):
        head, y = heads[name], r["ys"][name]
        head.train()
        head.head.eval()
        m.train()                                     # last: a head's train() reaches its .encoder too
        modes = [(mod, mod.training) for mod in head.modules()]
        params = list(head.parameters())
        before = [p.detach().clone() for p in params]
        passes = []
        real = fused_model.fused_encode
        fused_model.fused_encode = lambda *a, **kw: (passes.append(1), real(*a, **kw))[1]
        try:
            got = evaluate_finetune(head, _batches(tokens, y))
            again = evaluate_finetune(head, _batches(tokens, y))
        finally:
            fused_model.fused_encode = real
        assert "pbx_token_head_eval" in _lib._FN and "pbx_task_eval_fold" in _lib._FN     # not a fallback
        assert len(passes) == 2 * 3                                   # one encoder pass per batch
        assert got == again or str(got) == str(again)                 # bitwise repeatable (nan-safe)
        assert all(mod.training == t for mod, t in modes) and m.training and not head.head.training
        assert all(torch.equal(a, b) for a, b in zip(before, params)) and all(p.grad is None for p in params)
        # the confusion matrix of Predictor's calls
        lab = r["out"][f"task_{name}_labels"].long()
        live = y >= 0
        assert (lab[live] >= 0).all()
        want = torch.bincount(y[live] * K + lab[live], minlength=K * K).view(K, K)
        assert got["confusion"] == want.tolist()
        assert got["n"] == int(live.sum()) and got["n_batches"] == 3 and got["n_sequences"] == N
        assert got["accuracy"] == float(want.diag().sum()) / float(live.sum())
        assert got["support"] == want.sum(1).tolist() and got["predicted"] == want.sum(0).tolist()
        # the loss against F.cross_entropy on the model's own forward logits
        head.eval()
        total, budget = 0.0, 0.0
        with torch.no_grad():
            for tb, yb in _batches(tokens, y):
                z = head(tb.cuda()).float()                                               # [B, K, L]
                ce = F.cross_entropy(z, yb.cuda(), ignore_index=-100, reduction="none").double().cpu()
                n = int((yb >= 0).sum())
                total += float(ce.sum())
                budget += float(2 * ((18 + K) * EPS * n + EPS * ce.sum()) + 2 * n * EPS * ce.sum())
        err = abs(got["loss"] * got["n"] - total)
        print(f"{semantics} evaluate_finetune {name}: loss {got['loss']:.6f} err / budget {err / budget:.4f} "
              f"accuracy {got['accuracy']:.4f} macro_f1 {got['macro_f1']:.4f} mcc {got['mcc']:.4f}")
        assert err <= budget
        if name == "ss3":
            # a head built with dropout still takes the fused path (dropout is the identity in eval()): same bits
            torch.manual_seed(3)
            twin = ProteinBERTForTokenClassification(m, n_classes=3, freeze_encoder=False, hidden="all", dropout=0.3)
            twin.load_state_dict(head.state_dict())
            twin.train()
            _lib._FN.pop("pbx_token_head_eval")
            assert str(evaluate_finetune(twin, _batches(tokens, y))) == str(got)
            assert "pbx_token_head_eval" in _lib._FN and twin.dropout.training


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_per_protein_and_regression_heads_match_the_returned_states(semantics):
    from proteinbert_pytorch_replication_amd.train.evaluate_finetune import auroc, evaluate_finetune
    from proteinbert_pytorch_replication_amd.train.finetune import spearman
    r = _setup(semantics)
    heads, tokens, out = r["heads"], r["tokens"], r["out"]
    gen = torch.Generator().manual_seed(9)
    feats = {"loc": out["hidden_global"].reshape(N, BLOCKS * G), "bin": out["global"], "stab": out["global"]}
    for name, K in (("loc", 4), ("bin", 2)):
        z, d = _logits64(heads[name], feats[name])
        top = z.sort(-1, descending=True).values
        safe = (top[:, 0] - top[:, 1]) > 2 * d.max(-1).values
        assert safe.sum() >= N - 2
        y = torch.randint(0, K, (N,), generator=gen)
        y[:K] = torch.arange(K)                       # every class present
        y[~safe] = -1
        got = evaluate_finetune(heads[name], _batches(tokens, y))
        live = y >= 0
        want = torch.bincount(y[live] * K + z.argmax(-1)[live], minlength=K * K).view(K, K)
        assert got["confusion"] == want.tolist() and got["n"] == int(live.sum()) and got["n_sequences"] == N
        ce = (torch.logsumexp(z, -1) - z.gather(-1, y.clamp_min(0).unsqueeze(-1)).squeeze(-1))[live]
        assert abs(got["loss"] * got["n"] - float(ce.sum())) <= float((2 * d.max(-1).values[live] + 32 * EPS * (1 + ce)).sum())
        if K == 2:
            p1 = torch.softmax(z, -1)[:, 1]
            gaps = p1[live].sort().values.diff()
            ref = auroc(p1[live], y[live].double())
            print(f"{semantics} evaluate_finetune bin: auroc {got['auroc']:.6f} reference {ref:.6f}")
            if float(gaps.min()) > 4 * float(d.max()):            # the fp32 scores keep the fp64 order: same ranks
                assert got["auroc"] == ref
            assert abs(got["auroc"] - ref) <= 2.0 / N
    z, d = _logits64(heads["stab"], feats["stab"])
    t = torch.randn(N, generator=gen)
    got = evaluate_finetune(heads["stab"], _batches(tokens, t))
    p = z[:, 0]
    mse, mae = float(((p - t.double()) ** 2).mean()), float((p - t.double()).abs().mean())
    dm = float(d.max())
    assert got["n"] == N and got["n_batches"] == 3
    assert abs(got["mse"] - mse) <= 2 * dm * mae + dm * dm and abs(got["mae"] - mae) <= dm
    if float(p.sort().values.diff().min()) > 2 * dm:
        assert abs(got["spearman"] - spearman(p, t)) <= 1e-12
    assert abs(got["pearson"] - float(torch.corrcoef(torch.stack([p, t.double()]))[0, 1])) <= 1e-4
    print(f"{semantics} evaluate_finetune stab: mse {got['mse']:.6f} (fp64 {mse:.6f}) spearman {got['spearman']:.4f}")
