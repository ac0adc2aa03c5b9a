"""CPU: fine-tune evaluation (ops/task_eval.py, train/evaluate_finetune.py, ``finetune(evaluate="exact")``, ``cli
evaluate``) on the PyTorch backend: the metrics against hand-worked confusion matrices, the evaluation against a
direct computation for the three tasks in both semantics, model selection and early stopping, the untouched default
path, the CLI round trip and a 2-rank gloo evaluation."""
import json
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

from proteinbert_pytorch_replication_amd.data.synthetic import SyntheticSecondaryStructure, SyntheticSequenceTask
from proteinbert_pytorch_replication_amd.models import (ProteinBERT, ProteinBERTForSequenceClassification,
                                                        ProteinBERTForTokenClassification)
from proteinbert_pytorch_replication_amd.ops.task_eval import (TaskEvalAccumulator, class_counts_into,
                                                               metrics_from_confusion, scalar_metrics)
from proteinbert_pytorch_replication_amd.train.evaluate_finetune import auroc, evaluate_finetune, pearson
from proteinbert_pytorch_replication_amd.train.finetune import finetune, spearman

L, A, G, C, BLOCKS = 24, 40, 32, 16, 2
SMALL = ["model.sequences_length=32", "model.num_annotations=40", "model.local_dim=16", "model.global_dim=32",
         "model.key_dim=8", "model.num_blocks=2", "train.batch_size=4", "kernel.backend=torch", "kernel.dtype=fp32"]


def _enc(semantics="paper", seed=3):
    torch.manual_seed(seed)
    return ProteinBERT(sequences_length=L, num_annotations=A, local_dim=C, global_dim=G, key_dim=8, num_heads=2,
                       num_blocks=BLOCKS, device="cpu", semantics=semantics, backend="torch")


def _acc(cm, loss=0.0, bad=0, batches=1, seqs=1):
    K = len(cm)
    acc = TaskEvalAccumulator(K, "cpu")
    acc.counts[:K * K] = torch.tensor(cm).view(-1)
    acc.counts[K * K:] = torch.tensor([sum(map(sum, cm)), bad, batches, seqs])
    acc.loss[0] = loss
    return acc


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, rel=1e-14, abs=0)


def test_metrics_from_hand_worked_matrices():
    # class 2 absent from labels and predictions
    m = metrics_from_confusion(_acc([[5, 1, 0], [2, 3, 0], [0, 0, 0]], loss=22.0, batches=3, seqs=7))
    assert m["n"] == 11 and m["loss"] == 2.0 and m["accuracy"] == 8 / 11 and m["n_batches"] == 3 and m["n_sequences"] == 7
    assert m["support"] == [6, 5, 0] and m["predicted"] == [7, 4, 0] and m["confusion"] == [[5, 1, 0], [2, 3, 0], [0, 0, 0]]
    for got, want in ((m["precision"], [5 / 7, 3 / 4, math.nan]), (m["recall"], [5 / 6, 3 / 5, math.nan]),
                      (m["f1"], [10 / 13, 6 / 9, math.nan])):
        assert all(_same(g, w) for g, w in zip(got, want))
    assert _same(m["macro_f1"], (10 / 13 + 6 / 9) / 2)
    assert _same(m["weighted_f1"], (6 * 10 / 13 + 5 * 6 / 9) / 11)
    assert _same(m["mcc"], 26 / math.sqrt(56 * 60))
    # class 2 predicted and never true: precision 0, recall nan, F1 0, and it counts in the macro mean
    m = metrics_from_confusion(_acc([[5, 0, 1], [2, 3, 0], [0, 0, 0]]))
    assert m["precision"][2] == 0.0 and math.isnan(m["recall"][2]) and m["f1"][2] == 0.0
    assert _same(m["macro_f1"], (10 / 13 + 6 / 8 + 0.0) / 3)
    assert _same(m["weighted_f1"], (6 * 10 / 13 + 5 * 6 / 8) / 11)
    # 2 x 2: Gorodkin's coefficient is Matthews'
    m = metrics_from_confusion(_acc([[3, 1], [2, 4]]))
    assert m["accuracy"] == 0.7 and m["precision"] == [3 / 5, 4 / 5] and m["recall"] == [3 / 4, 4 / 6]
    assert _same(m["mcc"], (3 * 4 - 1 * 2) / math.sqrt(4 * 6 * 5 * 5))
    # a class with true rows and no true positive: F1 is 0, not nan
    m = metrics_from_confusion(_acc([[0, 2], [0, 3]]))
    assert m["f1"][0] == 0.0 and math.isnan(m["precision"][0]) and m["recall"][0] == 0.0
    # perfect and constant predictors
    assert metrics_from_confusion(_acc([[4, 0, 0], [0, 2, 0], [0, 0, 9]]))["mcc"] == 1.0
    assert math.isnan(metrics_from_confusion(_acc([[3, 0], [4, 0]]))["mcc"])
    # nothing counted: every ratio is nan
    m = metrics_from_confusion(_acc([[0, 0], [0, 0]], batches=0, seqs=0))
    assert m["n"] == 0 and all(math.isnan(m[k]) for k in ("loss", "accuracy", "macro_f1", "weighted_f1", "mcc"))
    assert all(math.isnan(v) for v in m["f1"] + m["precision"] + m["recall"])
    sm = scalar_metrics(m)
    assert set(sm) == {"n", "loss", "accuracy", "macro_f1", "weighted_f1", "mcc", "n_batches", "n_sequences"}
    json.dumps(sm)
    # bad labels are an error that names the count and the class count
    with pytest.raises(ValueError, match=r"2 labels.*n_classes=3"):
        metrics_from_confusion(_acc([[1, 0, 0], [0, 1, 0], [0, 0, 1]], bad=2))


def test_class_counts_into_row_classes():
    acc = TaskEvalAccumulator(3, "cpu")
    z = torch.tensor([[2.0, 1.0, 0.0], [0.0, 1.0, 1.0], [0.0, 0.0, 5.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    y = torch.tensor([0, 2, 1, -100, 3])
    class_counts_into(acc, z, y)
    assert acc.confusion.tolist() == [[1, 0, 0], [0, 0, 1], [0, 1, 0]]       # the tie calls the lower class
    assert acc.counts[9:].tolist() == [3, 1, 1, 5]
    want = F.cross_entropy(z[:3].double(), y[:3], reduction="sum")
    assert abs(acc.loss.item() - want.item()) < 1e-6


def _direct(model, batches, K):
    """Confusion, summed loss and live count from the model's own forward, batch by batch."""
    cm = torch.zeros(K, K, dtype=torch.int64)
    loss, n = 0.0, 0
    model.eval()
    with torch.no_grad():
        for X, y in batches:
            z = model(X).float()
            if z.dim() == 3:
                z, y = z.permute(0, 2, 1).reshape(-1, K), y.reshape(-1)
            live = y >= 0
            call = torch.softmax(z, -1).argmax(-1)
            cm += torch.bincount(y[live] * K + call[live], minlength=K * K).view(K, K)
            loss += float(F.cross_entropy(z[live], y[live], reduction="sum"))
            n += int(live.sum())
    return cm, loss, n


def _loader(ds, bs):
    return torch.utils.data.DataLoader(ds, batch_size=bs)


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_evaluate_finetune_against_a_direct_computation(semantics):
    enc = _enc(semantics)
    torch.manual_seed(11)
    n = 18
    tasks = [(ProteinBERTForTokenClassification(enc, n_classes=8, hidden="last"), SyntheticSecondaryStructure(n, L, 8, 4, seed=1)),
             (ProteinBERTForTokenClassification(enc, n_classes=3, hidden="all", use_global=False, dropout=0.2),
              SyntheticSecondaryStructure(n, L, 3, 4, seed=2)),
             (ProteinBERTForSequenceClassification(enc, n_classes=4, hidden="all"), SyntheticSequenceTask(n, L, 4, 4, seed=3)),
             (ProteinBERTForSequenceClassification(enc, n_classes=2), SyntheticSequenceTask(n, L, 2, 4, seed=4))]
    for model, ds in tasks:
        K = model.n_classes
        model.train()
        modes = [(m, m.training) for m in model.modules()]
        before = [p.detach().clone() for p in model.parameters()]
        res = {bs: evaluate_finetune(model, _loader(ds, bs)) for bs in (4, 7)}
        assert all(m.training == t for m, t in modes)
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
        assert all(p.grad is None for p in model.parameters())
        for bs, got in res.items():
            cm, loss, cnt = _direct(model, list(_loader(ds, bs)), K)
            model.train()
            assert got["confusion"] == cm.tolist() and got["n"] == cnt and got["n_sequences"] == n
            assert got["n_batches"] == -(-n // bs)
            assert abs(got["loss"] * cnt - loss) <= 1e-5 * loss
            assert got["accuracy"] == float(cm.diag().sum()) / cnt
        if semantics == "paper":                      # no batch-axis softmax anywhere: the batching is immaterial
            assert res[4]["confusion"] == res[7]["confusion"]
            assert abs(res[4]["loss"] - res[7]["loss"]) <= 1e-5 * res[4]["loss"]
        if K == 2:
            with torch.no_grad():
                model.eval()
                p1 = torch.cat([torch.softmax(model(X).float(), -1)[:, 1] for X, _ in _loader(ds, 4)])
                model.train()
            assert res[4]["auroc"] == auroc(p1, ds.labels) and 0.0 <= res[4]["auroc"] <= 1.0
            only = [(ds.tokens[:4], torch.ones(4, dtype=torch.int64))]
            assert math.isnan(evaluate_finetune(model, only)["auroc"])
    # regression
    model = ProteinBERTForSequenceClassification(enc, n_classes=1)
    ds = SyntheticSequenceTask(n, L, 1, 4, seed=5)
    got = evaluate_finetune(model, _loader(ds, 7))
    with torch.no_grad():
        model.eval()
        p = torch.cat([model(X).float().reshape(-1) for X, _ in _loader(ds, 7)]).double()
    t = ds.labels.double()
    assert got["n"] == n and got["n_batches"] == 3 and set(got) == {"n", "mse", "mae", "spearman", "pearson",
                                                                    "n_batches", "n_sequences"}
    assert got["mse"] == pytest.approx(float(((p - t) ** 2).mean()), rel=1e-12)
    assert got["mae"] == pytest.approx(float((p - t).abs().mean()), rel=1e-12)
    assert got["spearman"] == spearman(p, t) and got["pearson"] == pearson(p, t)
    assert got["pearson"] == pytest.approx(float(torch.corrcoef(torch.stack([p, t]))[0, 1]), rel=1e-9)
    # max_batches bounds the walk
    assert evaluate_finetune(model, _loader(ds, 7), max_batches=2)["n"] == 14


def test_auroc_average_ranks_on_ties():
    s = torch.tensor([0.1, 0.4, 0.4, 0.8, 0.4])
    y = torch.tensor([0, 0, 1, 1, 1])
    # pairs (pos, neg): 0.4 > 0.1, 0.4 = 0.4 (half), 0.8 > both, 0.4 > 0.1, 0.4 = 0.4 (half): 5 of 6
    assert auroc(s, y) == pytest.approx(5 / 6, rel=1e-15)


class _Scheduled:
    """A loader that sets the optimizer's learning rate for the epoch it is about to serve."""

    def __init__(self, loader, opt, lrs):
        self.loader, self.opt, self.lrs, self.epoch = loader, opt, lrs, 0

    def __iter__(self):
        for g in self.opt.param_groups:
            g["lr"] = self.lrs[min(self.epoch, len(self.lrs) - 1)]
        self.epoch += 1
        return iter(self.loader)


class _Snapshots:
    """A test loader that records the trainable parameters each time an evaluation starts."""

    def __init__(self, loader, model):
        self.loader, self.model, self.seen = loader, model, []

    def __iter__(self):
        self.seen.append([p.detach().clone() for p in self.model.parameters() if p.requires_grad])
        return iter(self.loader)


def test_finetune_exact_selects_the_best_epoch_and_stops_early():
    enc = _enc()
    torch.manual_seed(2)
    model = ProteinBERTForTokenClassification(enc, n_classes=3)
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
    train = _Scheduled(_loader(SyntheticSecondaryStructure(32, L, 3, 4, seed=1), 8), opt, [3e-2, 3e-2, 30.0, 30.0])
    test = _Snapshots(_loader(SyntheticSecondaryStructure(24, L, 3, 4, seed=2), 8), model)
    epochs, patience = 8, 2
    res = finetune(model, train, opt, epochs=epochs, test_dataloader=test, device="cpu", evaluate="exact",
                   select_metric="macro_f1", patience=patience)
    f1 = [m["macro_f1"] for m in res["test_eval"]]
    ran = len(f1)
    assert ran == len(res["train_loss"]) == len(res["test_loss"]) == len(res["test_metrics"]) == len(test.seen)
    best = max(range(ran), key=lambda e: (f1[e], -e))                   # the first epoch of the best value
    assert res["best_epoch"] == best and res["best_metric"] == f1[best]
    assert best < ran - 1, "the schedule was meant to make a later epoch worse"
    assert res["stopped_early"] is (ran < epochs) and res["stopped_early"] and ran == best + patience + 1
    got = [p for p in model.parameters() if p.requires_grad]
    assert all(torch.equal(a, b) for a, b in zip(got, test.seen[best]))
    assert not all(torch.equal(a, b) for a, b in zip(got, test.seen[-1]))
    assert res["test_loss"] == [m["loss"] for m in res["test_eval"]]
    assert res["test_metrics"] == [scalar_metrics(m) for m in res["test_eval"]]
    # a smaller-is-better metric, no patience: every epoch runs and the lowest loss is kept
    res = finetune(model, train, opt, epochs=2, test_dataloader=test, device="cpu", evaluate="exact", select_metric="loss")
    assert res["best_metric"] == min(res["test_loss"]) and res["stopped_early"] is False
    for kw in (dict(evaluate="exact", test_dataloader=None), dict(select_metric="loss"), dict(evaluate="nope"),
               dict(evaluate="exact", patience=2), dict(evaluate="exact", select_metric="f2")):
        with pytest.raises(ValueError):
            finetune(model, train, opt, epochs=1, device="cpu", **dict(dict(test_dataloader=test), **kw))


def test_finetune_default_path_is_untouched():
    def run():
        enc = _enc()
        torch.manual_seed(2)
        model = ProteinBERTForTokenClassification(enc, n_classes=3)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
        res = finetune(model, _loader(SyntheticSecondaryStructure(16, L, 3, 4, seed=1), 8), opt, epochs=2,
                       test_dataloader=_loader(SyntheticSecondaryStructure(12, L, 3, 4, seed=2), 8), device="cpu")
        return res, [p.detach().clone() for p in model.parameters()]
    (a, pa), (b, pb) = run(), run()
    assert set(a) == {"train_loss", "test_loss", "train_metrics", "test_metrics"}
    assert a == b and all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert all(set(m) == {"accuracy"} for m in a["test_metrics"])


def test_cli_finetune_exact_then_evaluate_round_trip(tmp_path, capsys):
    from proteinbert_pytorch_replication_amd.cli.__main__ import COMMANDS, main as cli_main
    from proteinbert_pytorch_replication_amd.cli.train import finetune_main
    from proteinbert_pytorch_replication_amd.train.checkpoint import save_final_model
    assert COMMANDS["evaluate"] == ("evaluate", "main")
    torch.manual_seed(5)
    enc = ProteinBERT(sequences_length=32, num_annotations=40, local_dim=16, global_dim=32, key_dim=8, num_heads=4,
                      num_blocks=2, device="cpu", backend="torch")
    (tmp_path / "pre").mkdir()
    model_path = save_final_model(enc, str(tmp_path / "pre"))
    res = finetune_main(["--preset", "cfg1_cpu_smoke", *SMALL, f"train.save_path={tmp_path / 'ft'}", "--pretrained",
                         model_path, "--epochs", "3", "--synthetic-samples", "64", "--classes", "HEC", "--lr", "3e-2",
                         "--eval", "exact", "--select-metric", "accuracy"])
    ft = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert ft["best_epoch"] == res["best_epoch"] and ft["test_eval"]["n"] == res["test_eval"][-1]["n"]
    assert set(ft) == {"train_loss", "test_metrics", "head", "test_eval", "best_epoch"}
    report = tmp_path / "report.json"
    cli_main(["evaluate", "--model", model_path, "--head", ft["head"], "--batch-size", "4", "--synthetic-samples", "64",
              "--classes", "HEC", "--n-classes", "3", "--out", str(report), "--backend", "torch", "--device", "cpu"])
    lines = capsys.readouterr().out.strip().splitlines()
    want = res["test_eval"][res["best_epoch"]]
    assert str(json.loads(lines[-1])) == str(scalar_metrics(want))
    assert str(json.loads(report.read_text())) == str(want)
    assert lines[0].split() == ["class", "support", "precision", "recall", "f1"] and lines[1].split()[0] == "H"
    assert any(ln.startswith("confusion") for ln in lines)
    # a CSV test set through the readers cli finetune uses
    csv = tmp_path / "t.csv"
    csv.write_text("seq,labels\nACDEFGHIKL,HHHEEECCCC\nMKVW,CCHH\n")
    cli_main(["evaluate", "--model", model_path, "--head", ft["head"], "--test-csv", str(csv), "--classes", "HEC",
              "--backend", "torch", "--device", "cpu"])
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert got["n"] == 14 and got["n_sequences"] == 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_models(enc):
    torch.manual_seed(13)
    return [(ProteinBERTForTokenClassification(enc, n_classes=3, hidden="all"), SyntheticSecondaryStructure(14, L, 3, 4, seed=1)),
            (ProteinBERTForSequenceClassification(enc, n_classes=2), SyntheticSequenceTask(14, L, 2, 4, seed=2)),
            (ProteinBERTForSequenceClassification(enc, n_classes=1), SyntheticSequenceTask(14, L, 1, 4, seed=3))]


def _shard(ds, lo, hi):
    return _loader(torch.utils.data.TensorDataset(ds.tokens[lo:hi], ds.labels[lo:hi]), 4)


def _eval_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from proteinbert_pytorch_replication_amd.parallel import dist as pdist
    pdist.init_distributed(device="cpu")
    got = [evaluate_finetune(m, _shard(ds, 0, 8) if rank == 0 else _shard(ds, 8, 14), distributed=True)
           for m, ds in _dist_models(_enc())]
    torch.save(got, os.path.join(out_dir, f"rank{rank}.pt"))
    pdist.destroy()


def test_distributed_evaluation_sums_over_ranks(tmp_path):
    """2-rank gloo, shards of 8 and 6 sequences in batches of 4: every rank returns the counts of one process that
    evaluates the same batches, exactly, and the same AUROC / Spearman."""
    world = 2
    mp.start_processes(_eval_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, start_method="spawn",
                       join=True)
    torch.set_num_threads(1)
    ref = [evaluate_finetune(m, list(_shard(ds, 0, 8)) + list(_shard(ds, 8, 14))) for m, ds in _dist_models(_enc())]
    for r in range(world):
        got = torch.load(tmp_path / f"rank{r}.pt", weights_only=False)
        tok, seq, reg = got
        for k in ("confusion", "n", "n_batches", "n_sequences", "support", "predicted", "accuracy", "macro_f1", "mcc"):
            assert str(tok[k]) == str(ref[0][k]), k
            assert str(seq[k]) == str(ref[1][k]), k
        assert abs(tok["loss"] - ref[0]["loss"]) <= 1e-6 * ref[0]["loss"]
        assert seq["auroc"] == ref[1]["auroc"]
        assert reg["n"] == 14 and reg["n_batches"] == 4 and reg["spearman"] == ref[2]["spearman"]
        assert reg["mse"] == ref[2]["mse"] and reg["pearson"] == ref[2]["pearson"]
