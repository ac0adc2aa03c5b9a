"""Held-out evaluation on the PyTorch path (train/evaluate.py): ``evaluate_pretrain`` against a hand-written
computation for both semantics, ``pretrain(..., eval_every=...)`` leaving the training run bitwise unchanged,
the ``cli pretrain`` wiring (``eval.every``) and the 2-rank all-reduce of the accumulator."""
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from proteinbert_pytorch_replication_amd.data import CorruptionParams, SyntheticUniRefGO
from proteinbert_pytorch_replication_amd.models import ProteinBERT
from proteinbert_pytorch_replication_amd.train.evaluate import evaluate_pretrain, metrics_from_accumulator
from proteinbert_pytorch_replication_amd.train.losses import pretrain_loss_torch
from proteinbert_pytorch_replication_amd.train.pretrain import pretrain
from proteinbert_pytorch_replication_amd.utils import determinism

CFG = dict(sequences_length=32, num_annotations=40, local_dim=16, global_dim=32, key_dim=8, num_heads=4,
           num_blocks=2)
COUNT_KEYS = ("n_batches", "n_sequences", "n_tokens", "n_masked_tokens", "n_go_pos", "n_go_neg")


def _model(semantics="reference", seed=0):
    torch.manual_seed(seed)
    return ProteinBERT(backend="torch", semantics=semantics, **CFG)


def _batches(n, seed, B=5):
    """Synthetic batches with a zero-weight pad tail (lengths well below L) and all-blank annotation rows
    (weight 0 over the whole row)."""
    gen = SyntheticUniRefGO(CFG["sequences_length"], CFG["num_annotations"], B, "cpu", seed=seed, max_length=24,
                            density=0.1, use_kernel=False, corruption=CorruptionParams(token_p=0.3))
    out = []
    for i in range(n):
        X, Y, W = gen.next_batch()
        ann = Y["global"].clone()
        ann[i % B] = 0                                  # an all-blank row: w_global = any(ann) = 0
        Y = dict(Y, **{"global": ann})
        W = dict(W, **{"global": (ann != 0).any(dim=1, keepdim=True).float().expand_as(ann)})
        assert (W["local"][:, -1] == 0).all() and (W["global"][i % B] == 0).all() and (W["global"] > 0).any()
        assert (X["local"] != Y["local"]).any()
        out.append((X, Y, W))
    return out


def _by_hand(m, batches):
    """Plain loops over numpy arrays: losses through pretrain_loss_torch, every count one entry at a time."""
    ll = lg = 0.0
    c = dict.fromkeys(COUNT_KEYS, 0)
    hits = mhits = tp = fp = 0
    hp, hn = [0] * 256, [0] * 256
    with torch.no_grad():
        for X, Y, W in batches:
            pl, pg = m.heads_torch(*m.encode_torch(X["local"], X["global"]))
            _, a, b = pretrain_loss_torch(pl, pg, Y, W, m.semantics, return_parts=True)
            ll += float(a)
            lg += float(b)
            P, x, y, w = pl.numpy(), X["local"].numpy(), Y["local"].numpy(), W["local"].numpy()
            c["n_batches"] += 1
            c["n_sequences"] += P.shape[0]
            for i in range(P.shape[0]):
                for j in range(P.shape[1]):
                    if w[i, j] <= 0:
                        continue
                    best = 0
                    for v in range(1, P.shape[2]):
                        if P[i, j, v] > P[i, j, best]:
                            best = v
                    c["n_tokens"] += 1
                    hits += best == y[i, j]
                    if x[i, j] != y[i, j]:
                        c["n_masked_tokens"] += 1
                        mhits += best == y[i, j]
            p, yg, wg = pg.float().numpy(), Y["global"].numpy(), W["global"].numpy()
            for i in range(p.shape[0]):
                for k in range(p.shape[1]):
                    if wg[i, k] <= 0:
                        continue
                    b_ = min(255, int(np.float32(p[i, k]) * np.float32(256)))
                    if yg[i, k] == 1:
                        hp[b_] += 1
                        tp += p[i, k] >= 0.5
                    else:
                        hn[b_] += 1
                        fp += p[i, k] >= 0.5
    c["n_go_pos"], c["n_go_neg"] = sum(hp), sum(hn)
    n = len(batches)
    return dict(c, loss_local=ll / n, loss_global=lg / n, loss=(ll + lg) / n, hits=int(hits), mhits=int(mhits),
                tp=int(tp), fp=int(fp), hp=hp, hn=hn)


@pytest.mark.parametrize("semantics", ["reference", "paper"])
def test_evaluate_matches_hand_computation(semantics):
    m = _model(semantics)
    batches = _batches(3, seed=11)
    m.train()
    got = evaluate_pretrain(m, batches)
    assert m.training                                    # the previous mode is restored
    ref = _by_hand(m, batches)
    for k in COUNT_KEYS:
        assert got[k] == ref[k], k
    assert got["go_hist_pos"].tolist() == ref["hp"] and got["go_hist_neg"].tolist() == ref["hn"]
    assert got["go_hist_pos"].dtype == torch.int64
    for k in ("loss", "loss_local", "loss_global"):
        assert got[k] == pytest.approx(ref[k], rel=1e-12), k
    assert got["token_accuracy"] == ref["hits"] / ref["n_tokens"]
    assert ref["n_masked_tokens"] > 0 and got["masked_token_accuracy"] == ref["mhits"] / ref["n_masked_tokens"]
    # threshold 0.5 = bin 128 exactly: the histogram metrics equal the ones counted from p >= 0.5
    tp, fp, npos = ref["tp"], ref["fp"], ref["n_go_pos"]
    assert npos > 0 and ref["n_go_neg"] > 0
    assert got["go_recall"] == tp / npos
    assert got["go_precision"] == pytest.approx(tp / (tp + fp)) if tp + fp else math.isnan(got["go_precision"])
    assert got["go_f1"] == pytest.approx(2 * tp / (2 * tp + fp + npos - tp))
    # Mann-Whitney over the bins, pair by pair
    u = 0.0
    for a in range(256):
        for b in range(256):
            u += ref["hp"][a] * ref["hn"][b] * (1.0 if a > b else 0.5 if a == b else 0.0)
    assert got["go_auroc"] == pytest.approx(u / (npos * ref["n_go_neg"]), rel=1e-12)
    # max_batches bounds the loader
    assert evaluate_pretrain(m, batches, max_batches=2)["n_batches"] == 2


def test_metrics_nan_on_empty_denominators():
    got = metrics_from_accumulator(torch.zeros(2, dtype=torch.float64), torch.zeros(520, dtype=torch.int64))
    for k in ("loss", "token_accuracy", "masked_token_accuracy", "go_precision", "go_recall", "go_f1", "go_auroc"):
        assert math.isnan(got[k]), k
    assert got["n_tokens"] == 0 and got["n_go_pos"] == 0


class _Loader:
    """Endless training loader / bounded held-out loader over one generator."""

    def __init__(self, seed, n=None):
        self.gen = SyntheticUniRefGO(CFG["sequences_length"], CFG["num_annotations"], 4, "cpu", seed=seed,
                                     use_kernel=False)
        self.n = n

    def __iter__(self):
        i = 0
        while self.n is None or i < self.n:
            yield self.gen.next_batch()
            i += 1


def _pretrain_run(tmp, with_eval):
    m = _model(seed=5)
    torch.manual_seed(1)
    kw = dict(eval_dataloader=_Loader(77), eval_every=2, eval_batches=2) if with_eval else {}
    res = pretrain(m, _Loader(3), torch.optim.Adam(m.parameters(), lr=1e-3), max_batch_iterations=4,
                   save_path=str(tmp), nb_iterations_checkpoint=100, warmup_duration=2, final_save=False,
                   metrics_path=str(tmp / "m.jsonl"), tensorboard_dir=str(tmp / "tb"), **kw)
    state = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    return res, state, torch.get_rng_state()


def test_pretrain_eval_leaves_training_bitwise_unchanged(tmp_path):
    prev = torch.are_deterministic_algorithms_enabled()
    determinism.enable()
    try:
        (tmp_path / "a").mkdir()
        (tmp_path / "b").mkdir()
        r0, p0, rng0 = _pretrain_run(tmp_path / "a", False)
        r1, p1, rng1 = _pretrain_run(tmp_path / "b", True)
    finally:
        torch.use_deterministic_algorithms(prev)
        determinism._STATE["on"] = False
    assert torch.equal(p0, p1)
    assert r0["train_loss"] == r1["train_loss"] and len(r1["train_loss"]) == 4
    assert torch.equal(rng0, rng1)                       # the training RNG stream is where it would have been
    assert "eval" not in r0
    assert [e["step"] for e in r1["eval"]] == [2, 4]
    for e in r1["eval"]:
        assert e["n_batches"] == 2 and e["n_sequences"] == 8 and math.isfinite(e["loss"])
        assert 0.0 <= e["token_accuracy"] <= 1.0
    recs = [json.loads(ln) for ln in open(tmp_path / "b" / "m.jsonl")]
    ev = [r for r in recs if "eval_loss" in r]
    assert [r["step"] for r in ev] == [2, 4]
    assert ev[1]["eval_loss"] == r1["eval"][1]["loss"] and "eval_go_auroc" in ev[0] and "eval_n_tokens" in ev[0]
    assert len([r for r in recs if "loss" in r]) == 4    # the training records are all still there
    assert not any("eval_loss" in json.loads(ln) for ln in open(tmp_path / "a" / "m.jsonl"))
    assert os.listdir(tmp_path / "b" / "tb")


def test_pretrain_cli_eval_every(tmp_path, capsys):
    from proteinbert_pytorch_replication_amd.cli.train import pretrain_main
    small = ["model.sequences_length=32", "model.num_annotations=40", "model.local_dim=16", "model.global_dim=32",
             "model.key_dim=8", "model.num_blocks=1", "train.batch_size=4", "kernel.backend=torch",
             "kernel.dtype=fp32", "optim.warmup_duration=2", "train.nb_iterations_checkpoint=100"]
    pretrain_main(["--preset", "cfg1_cpu_smoke", *small, f"train.save_path={tmp_path}", "train.max_batch_iterations=4",
                   "eval.every=2", "eval.batches=3", "eval.seed=9", "--resume", "none", "--log-every", "1",
                   "--metrics", str(tmp_path / "m.jsonl")])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["iterations"] == 4
    assert out["eval"]["n_batches"] == 3 and out["eval"]["n_sequences"] == 12
    ev = [json.loads(ln) for ln in open(tmp_path / "m.jsonl")]
    assert [r["step"] for r in ev if "eval_loss" in r] == [2, 4]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _eval_worker(rank, world, port, out_dir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from proteinbert_pytorch_replication_amd.parallel import dist as pdist
    pdist.init_distributed(device="cpu")
    m = _model("paper")
    got = evaluate_pretrain(m, _batches(2, seed=20 + rank), distributed=True)
    torch.save(got, os.path.join(out_dir, f"rank{rank}.pt"))
    pdist.destroy()


def test_distributed_evaluation_sums_over_ranks(tmp_path):
    """2-rank gloo, paper semantics: every rank returns the counts and histograms of one process evaluating
    both ranks' batches, exactly, and the same loss."""
    world = 2
    mp.start_processes(_eval_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, start_method="spawn",
                       join=True)
    ref = evaluate_pretrain(_model("paper"), _batches(2, seed=20) + _batches(2, seed=21))
    for r in range(world):
        got = torch.load(tmp_path / f"rank{r}.pt", weights_only=True)
        for k in COUNT_KEYS:
            assert got[k] == ref[k], k
        assert torch.equal(got["go_hist_pos"], ref["go_hist_pos"]) and torch.equal(got["go_hist_neg"], ref["go_hist_neg"])
        for k in ("loss", "loss_local", "loss_global"):
            assert abs(got[k] - ref[k]) <= 1e-6 * abs(ref[k]), k
        assert got["token_accuracy"] == ref["token_accuracy"] and got["go_auroc"] == ref["go_auroc"]
