"""The residue fine-tuning loss (train/task_loss.py): class weights and label smoothing, on the torch backend.

``ResidueTaskLoss`` against ``F.cross_entropy`` in fp64 and against the closed forms of its docstring (loss and
logit gradient); ``balanced_class_weights`` by hand; ``model.loss`` against ``loss_fn(model(x), y)`` and
``token_accuracy``; which loop ``train_step`` takes; the command line."""
import copy
import json
import math

import pytest
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

from proteinbert_pytorch_replication_amd.cli.train import finetune_main
from proteinbert_pytorch_replication_amd.data.synthetic import SyntheticSecondaryStructure
from proteinbert_pytorch_replication_amd.models import ProteinBERT, ProteinBERTForTokenClassification
from proteinbert_pytorch_replication_amd.ops import finetune_head
from proteinbert_pytorch_replication_amd.train import finetune as ft
from proteinbert_pytorch_replication_amd.train.finetune import finetune, token_accuracy
from proteinbert_pytorch_replication_amd.train.task_loss import ResidueTaskLoss, balanced_class_weights

F64 = torch.float64
NB, C, G, L, A, K = 3, 32, 64, 32, 48, 5
SMALL = ["model.sequences_length=32", "model.num_annotations=64", "model.local_dim=16", "model.global_dim=32",
         "model.key_dim=8", "model.num_heads=4", "model.num_blocks=2", "train.batch_size=4", "kernel.backend=torch"]
WEIGHTS = [0.3, 1.0, 0.0, 2.5, 0.7]


def _encoder(semantics="reference", seed=0):
    torch.manual_seed(seed)
    return ProteinBERT(sequences_length=L, num_annotations=A, local_dim=C, global_dim=G, key_dim=16, num_heads=2,
                       num_blocks=NB, device="cpu", backend="torch", semantics=semantics)


def _batch(B=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, L, generator=g) * 2
    y = torch.randint(0, K, (B, L), generator=g)
    y[torch.rand(B, L, generator=g) < 0.3] = -100
    y[0] = -100
    return z, y


@pytest.mark.parametrize("weights", [None, WEIGHTS])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_loss_matches_fp64_cross_entropy_and_the_closed_forms(weights, eps):
    z, y = _batch()
    loss_fn = ResidueTaskLoss(weights, eps)
    zg = z.clone().requires_grad_(True)
    got = loss_fn(zg, y)
    got.backward()
    z64 = z.to(F64).requires_grad_(True)
    w64 = None if weights is None else torch.tensor(weights, dtype=F64)
    ref = F.cross_entropy(z64, y, weight=w64, ignore_index=-100, label_smoothing=eps)
    ref.backward()
    assert got.dtype == torch.float32 and abs(got.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert (zg.grad.to(F64) - z64.grad).abs().max().item() <= 1e-6
    # the closed forms of the module docstring, in fp64
    Z = z.to(F64).permute(0, 2, 1).reshape(-1, K)
    yf = y.reshape(-1)
    live = yf >= 0
    w = torch.ones(K, dtype=F64) if w64 is None else w64
    lp = torch.log_softmax(Z, -1)
    p = lp.exp()
    ys = yf.clamp_min(0)
    wy = w[ys] * live
    onehot = F.one_hot(ys, K).to(F64)
    rows = (1 - eps) * wy * -(lp.gather(-1, ys[:, None])[:, 0]) + (eps / K) * live * (w * -lp).sum(-1)
    g = (1 - eps) * wy[:, None] * (p - onehot) + (eps / K) * live[:, None] * (p * w.sum() - w)
    # torch may carry label_smoothing as an fp32 number (0.1 is then off by 1.5e-9): 1e-8 covers that, and with
    # eps = 0 the agreement is that of fp64
    tol = 1e-8 if eps else 1e-13
    assert abs((rows.sum() / wy.sum()).item() - ref.item()) <= tol * abs(ref.item())
    gref = z64.grad.permute(0, 2, 1).reshape(-1, K)
    assert (g / wy.sum() - gref).abs().max().item() <= tol


def test_an_all_ignored_batch_has_a_nan_loss_and_a_zero_gradient():
    z, y = _batch()
    zg = z.clone().requires_grad_(True)
    loss = ResidueTaskLoss(WEIGHTS, 0.1)(zg, torch.full_like(y, -100))
    loss.backward()
    assert math.isnan(loss.item()) and not zg.grad.any()


def test_constructor_rejects_bad_arguments():
    for eps in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ResidueTaskLoss(label_smoothing=eps)
    for cw in ([], [1.0, -1.0], [float("nan")], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            ResidueTaskLoss(cw)
    z, y = _batch()
    with pytest.raises(ValueError):
        ResidueTaskLoss([1.0, 2.0])(z, y)                      # two weights for five classes
    assert isinstance(ResidueTaskLoss(), torch.nn.Module) and ResidueTaskLoss().class_weights is None


def test_balanced_class_weights_by_hand():
    labels = torch.tensor([[0, 0, 0, 0, 0, 0], [1, 1, 1, 3, -100, -100]])
    w = balanced_class_weights(labels, 4)
    assert w.dtype == torch.float32 and w.shape == (4,)
    assert torch.equal(w, torch.tensor([10 / 24, 10 / 12, 0.0, 10 / 4], dtype=torch.float64).float())
    # an iterable of label batches is the same pass; a balanced set gets ones; an empty one zeros
    assert torch.equal(balanced_class_weights(iter([labels[0], labels[1]]), 4), w)
    assert torch.equal(balanced_class_weights(torch.arange(12) % 3, 3), torch.ones(3))
    assert torch.equal(balanced_class_weights(torch.full((5,), -100), 3), torch.zeros(3))
    with pytest.raises(ValueError, match="outside"):
        balanced_class_weights(torch.tensor([0, 4]), 4)


@pytest.mark.parametrize("semantics", ["reference", "paper"])
@pytest.mark.parametrize("hidden", ["last", "all"])
def test_model_loss_is_loss_of_forward_and_token_accuracy(semantics, hidden):
    model = ProteinBERTForTokenClassification(_encoder(semantics), n_classes=K, hidden=hidden).train()
    g = torch.Generator().manual_seed(5)
    x = {"local": torch.randint(4, 26, (4, L), generator=g), "global": (torch.rand(4, A, generator=g) < 0.1).float()}
    y = torch.randint(0, K, (4, L), generator=g)
    y[torch.rand(4, L, generator=g) < 0.3] = -100
    loss_fn = ResidueTaskLoss(WEIGHTS, 0.1)
    loss, acc = model.loss(x, y, loss_fn)
    logits = model(x)
    want = loss_fn(logits, y)
    want_acc = token_accuracy()(torch.softmax(logits.detach().float(), dim=1), y)
    assert torch.equal(loss, want) and torch.equal(acc, want_acc) and loss.requires_grad and not acc.requires_grad
    n_live = int((y >= 0).sum())
    assert loss_fn.counter("cpu").tolist() == [n_live, round(float(want_acc) * n_live), 0]
    gl = torch.autograd.grad(loss, model.head.weight)[0]
    gw = torch.autograd.grad(want, model.head.weight)[0]
    assert torch.equal(gl, gw)
    with pytest.raises(ValueError, match="class weights"):
        model.loss(x, y, ResidueTaskLoss([1.0, 2.0]))


def _run(loss_fn, metrics=None, epochs=2, labels=None):
    enc = _encoder()
    torch.manual_seed(11)
    model = ProteinBERTForTokenClassification(enc, n_classes=K)
    ds = SyntheticSecondaryStructure(16, L, K, seed=2)
    if labels is not None:
        ds.labels = labels(ds.labels.clone())
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
    res = finetune(model, DataLoader(ds, batch_size=4), opt, epochs=epochs, loss_fn=loss_fn, metrics=metrics,
                   device="cpu")
    return res, model


def test_default_loss_is_bitwise_the_cross_entropy_loop():
    ra, ma = _run(None)
    rb, mb = _run(torch.nn.CrossEntropyLoss(ignore_index=-100))
    assert ra["train_loss"] == rb["train_loss"] and ra["train_metrics"] == rb["train_metrics"]
    for (ka, pa), (kb, pb) in zip(ma.state_dict().items(), mb.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb)
    # the unshaped ResidueTaskLoss is the same objective (through model.loss)
    rc, _ = _run(ResidueTaskLoss())
    assert rc["train_loss"] == pytest.approx(ra["train_loss"], rel=1e-6)
    assert rc["train_metrics"][0]["accuracy"] == pytest.approx(ra["train_metrics"][0]["accuracy"], rel=1e-6)


def test_train_step_takes_model_loss_only_for_tagged_metrics(monkeypatch):
    calls = []
    real = ProteinBERTForTokenClassification.loss
    monkeypatch.setattr(ProteinBERTForTokenClassification, "loss",
                        lambda self, x, y, loss: (calls.append(1), real(self, x, y, loss))[1])
    loss_fn = ResidueTaskLoss(WEIGHTS, 0.1)
    r1, _ = _run(copy.deepcopy(loss_fn), epochs=1)
    assert len(calls) == 4                                        # 16 samples in batches of 4: the model.loss loop
    del calls[:]
    custom = {"accuracy": token_accuracy(), "live": lambda preds, y: (y != -100).float().mean()}
    r2, _ = _run(copy.deepcopy(loss_fn), metrics=custom, epochs=1)
    assert not calls and set(r2["train_metrics"][0]) == {"accuracy", "live"}
    assert r2["train_loss"] == pytest.approx(r1["train_loss"], rel=1e-6)
    assert r2["train_metrics"][0]["accuracy"] == pytest.approx(r1["train_metrics"][0]["accuracy"], rel=1e-6)
    # another ignore_index than the loss's, or a loss that is not a ResidueTaskLoss: the loop on the logits
    _run(copy.deepcopy(loss_fn), metrics={"accuracy": token_accuracy(-1)}, epochs=1)
    _run(torch.nn.CrossEntropyLoss(ignore_index=-100), epochs=1)
    assert not calls
    assert token_accuracy(-7).token_accuracy_ignore_index == -7
    assert ft._fused_loss_step(object(), loss_fn, {}) is False


def test_labels_outside_the_classes_raise_at_the_end_of_the_epoch():
    def plant(lab):
        live = (lab >= 0).nonzero()
        for i, j in live[[0, 5, 9]].tolist():
            lab[i, j] = K + (i % 2) * 1000
        return lab
    with pytest.raises(ValueError, match=r"^3 training labels"):
        _run(ResidueTaskLoss(WEIGHTS, 0.1), epochs=1, labels=plant)


def test_fused_switch_and_support_condition_exist():
    assert finetune_head.LOSS_FUSED is True
    h = torch.zeros(2, 8, 128, dtype=torch.bfloat16)
    assert finetune_head.supported_loss([h], 8) is finetune_head.supported_multi([h], 8) is False   # CPU rows
    loss, acc = finetune_head.token_head_loss_torch([h.float()], torch.zeros(3, 128), torch.tensor([0.0, 1.0, 1.0]),
                                                    None, torch.tensor([[1] * 4 + [2] * 3 + [-100]] * 2),
                                                    torch.tensor([1.0, 2.0, 1.0]), 0.0)
    # logits (0, 1, 1): classes 1 and 2 tie and the lower one is called; ce = log(2 + 1/e) for both labels
    assert acc.item() == pytest.approx(4 / 7) and loss.item() == pytest.approx(math.log(2 + math.exp(-1.0)), rel=1e-6)


def test_cli_balanced_weights_and_smoothing(tmp_path, capsys):
    res = finetune_main(["--preset", "cfg1_cpu_smoke", *SMALL, f"train.save_path={tmp_path}", "--epochs", "2",
                         "--synthetic-samples", "32", "--class-weights", "balanced", "--label-smoothing", "0.1",
                         "--eval", "exact", "--select-metric", "macro_f1"])
    summary = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert summary["loss"]["label_smoothing"] == 0.1 and len(summary["loss"]["class_weights"]) == 3
    assert all(w > 0 for w in summary["loss"]["class_weights"])
    assert len(res["train_loss"]) == 2 and all(math.isfinite(v) for v in res["train_loss"])
    assert "macro_f1" in summary["test_eval"] and summary["best_epoch"] in (0, 1)
    # the head file keeps its format: tensors only for the default form
    head = torch.load(summary["head"])
    assert set(head) == {"head.weight", "head.bias", "global_head.weight"}


def test_cli_explicit_weights_fused_flag_and_rejections(tmp_path, capsys):
    base = ["--preset", "cfg1_cpu_smoke", *SMALL, f"train.save_path={tmp_path}", "--epochs", "1",
            "--synthetic-samples", "16"]
    finetune_main(base + ["--class-weights", "1,2,0.5"])
    s = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert s["loss"] == {"class_weights": [1.0, 2.0, 0.5], "label_smoothing": 0.0}
    finetune_main(base + ["--fused-loss"])
    assert "loss" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    finetune_main(base)
    assert "loss" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with pytest.raises(ValueError, match="2 weights for the 3 classes"):
        finetune_main(base + ["--class-weights", "1,2"])
    with pytest.raises(ValueError, match="expected 'balanced'"):
        finetune_main(base + ["--class-weights", "heavy"])
    with pytest.raises(ValueError, match="label-smoothing"):
        finetune_main(base + ["--label-smoothing", "1.0"])
    for flags in (["--class-weights", "balanced"], ["--label-smoothing", "0.1"], ["--fused-loss"]):
        with pytest.raises(ValueError, match="need --task residue"):
            finetune_main(base + ["--task", "sequence", *flags])
        with pytest.raises(ValueError, match="need --task residue"):
            finetune_main(base + ["--task", "regression", *flags])
