"""``evaluate``: whole-set metrics of a fine-tuned head on a labelled test set.

    python -m proteinbert_pytorch_replication_amd.cli evaluate --model enc.pt --head head.pt --test-csv x.csv \\
        [--classes HEC] [--n-classes N] [--batch-size N] [--out report.json]

The model is a file written by ``train.checkpoint.save_final_model`` (or a training checkpoint holding the
model's config), the head a ``proteinbert_finetuned_head.pt`` of ``cli finetune``; the CSV has the columns
``cli finetune`` reads for the head's task (``seq`` and ``labels`` for a residue head, ``seq`` and ``label``
otherwise).  Without ``--test-csv`` the task's synthetic test set is evaluated, the one ``cli finetune`` draws
(``--synthetic-samples``, ``--seed``).  Prints a per-class table (class, support, precision, recall, F1) and the
confusion matrix (true x predicted) for a classification head, then the scalar metrics as one JSON line;
``--out`` writes the full dict (:func:`..train.evaluate_finetune.evaluate_finetune`).  For a reference-semantics
encoder the numbers depend on ``--batch-size``, as every evaluation of such a model does.
"""
from __future__ import annotations

import argparse
import json
from typing import List, Optional

import torch

from ..models.finetune import load_finetuned_head
from ..train.checkpoint import load_model
from ..train.evaluate_finetune import evaluate_finetune, scalar_metrics


def _table(m: dict, names: List[str]) -> str:
    K = len(names)
    w = max(5, *(len(n) for n in names))
    lines = [f"{'class':>{w}} {'support':>9} {'precision':>9} {'recall':>9} {'f1':>9}"]
    for k in range(K):
        lines.append(f"{names[k]:>{w}} {m['support'][k]:>9d} {m['precision'][k]:>9.4f} {m['recall'][k]:>9.4f} "
                     f"{m['f1'][k]:>9.4f}")
    cw = max(w, *(len(str(v)) for row in m["confusion"] for v in row))
    lines.append("confusion (rows: true, columns: predicted)")
    lines.append(" " * (w + 1) + " ".join(f"{n:>{cw}}" for n in names))
    for k in range(K):
        lines.append(f"{names[k]:>{w}} " + " ".join(f"{v:>{cw}d}" for v in m["confusion"][k]))
    return "\n".join(lines)


def main(argv: Optional[List[str]] = None) -> dict:
    ap = argparse.ArgumentParser(prog="evaluate", description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="saved encoder (.pt)")
    ap.add_argument("--head", required=True, help="fine-tuned head file (cli finetune)")
    ap.add_argument("--test-csv", default=None, help="labelled test set (default: the task's synthetic test set)")
    ap.add_argument("--classes", default=None, help="residue head: label alphabet (default: the head file's, else HEC)")
    ap.add_argument("--n-classes", type=int, default=None, help="checked against the head's class count")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--out", default=None, help="write the full metrics dict as JSON")
    ap.add_argument("--synthetic-samples", type=int, default=2048, help="as cli finetune: the test set is 1/8 of it")
    ap.add_argument("--seed", type=int, default=0, help="as cli finetune's train.seed (synthetic test set)")
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is a GPU, else cpu")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])
    a = ap.parse_args(argv)
    device = torch.device(a.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    enc = load_model(a.model, device=device, backend=a.backend)
    model, meta = load_finetuned_head(a.head, enc)
    model.to(device)
    K, task = meta["n_classes"], meta["task"]
    if a.n_classes is not None and a.n_classes != K:
        raise SystemExit(f"--n-classes {a.n_classes}: the head has {K} classes")
    classes = a.classes or meta.get("classes") or ("HEC" if task == "residue" and K == 3 else None)
    if task == "residue" and classes is not None and len(classes) != K:
        raise SystemExit(f"--classes {classes!r} has {len(classes)} letters, the head {K} classes")
    L = enc.config["sequences_length"]
    from .train import _seq_csv, _ss_csv
    from ..data.synthetic import SyntheticSecondaryStructure, SyntheticSequenceTask
    if a.test_csv:
        if task == "residue":
            if classes is None:
                raise SystemExit("a residue head without a class alphabet in its file needs --classes")
            ds = _ss_csv(a.test_csv, L, classes)
        else:
            ds = _seq_csv(a.test_csv, L, task == "regression", K)
    elif task == "residue":
        ds = SyntheticSecondaryStructure(max(64, a.synthetic_samples // 8), L, K, seed=a.seed + 1)
    else:
        ds = SyntheticSequenceTask(max(64, a.synthetic_samples // 8), L, K, seed=a.seed + 1)
    m = evaluate_finetune(model, torch.utils.data.DataLoader(ds, batch_size=a.batch_size), device=device)
    if "confusion" in m:
        names = list(classes) if task == "residue" and classes is not None else [str(k) for k in range(K)]
        print(_table(m, names))
    print(json.dumps(scalar_metrics(m)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(m, f)
    return m


if __name__ == "__main__":
    main()
