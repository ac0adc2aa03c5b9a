"""``predict``: embeddings, GO-term predictions and residue calls for the records of a FASTA file.

    python -m proteinbert_pytorch_replication_amd.cli predict --model model.pt --fasta in.fasta --out out.npz \\
        [--outputs global,pooled,go_topk] [--go-top-k K] [--attention-top-k K] [--batch-size N] [--truncate] \\
        [--head NAME=head.pt ...] [--head-classes NAME=ALPHABET ...]

The model is a file written by ``train.checkpoint.save_final_model`` (or a training checkpoint holding the
model's config); the ``.npz`` holds ``ids`` (the FASTA record names, in file order) and the arrays of the
requested outputs (:mod:`..inference`).  bf16 arrays are stored as fp32.  For a reference-semantics model
the residue probabilities and calls depend on ``--batch-size`` (see :mod:`..inference`).  ``--outputs
attention,attention_top`` (paper-semantics models only) stores the attention maps ``attention [N, blocks, H, L]``
and the ``--attention-top-k`` most attended positions per block and head (``attention_top_values`` /
``attention_top_indices``).

``--head NAME=PATH`` (repeatable) registers a head file of ``cli finetune`` and adds its ``task:NAME`` output:
``task_NAME_labels`` / ``task_NAME_label_probs`` (``task_NAME_values`` for a regression head), and
``task_NAME_probs`` when ``task_probs:NAME`` is among ``--outputs``.  A residue head with a class alphabet (the
file's ``meta["classes"]``, or ``--head-classes NAME=ALPHABET``) also gives ``task_NAME_string``: one string per
record, one class letter per residue, of the record's own length.  The head of a ``finetune --unfreeze`` run goes
with the encoder file that run saved (``--model``).
"""
from __future__ import annotations

import argparse
import json
from typing import Dict, List, Optional

import numpy as np
import torch

from ..etl.fasta import FastaIndex
from ..inference import DEFAULT_OUTPUTS, OUTPUTS, Predictor
from ..models import ProteinBERTForTokenClassification
from ..train.checkpoint import load_model


def _pairs(items: List[str], flag: str) -> Dict[str, str]:
    """``NAME=VALUE`` arguments of a repeatable flag as a dict."""
    out: Dict[str, str] = {}
    for it in items:
        name, sep, value = it.partition("=")
        if not sep or not name or not value:
            raise SystemExit(f"{flag} {it!r}: expected NAME=VALUE")
        if name in out:
            raise SystemExit(f"{flag}: {name!r} given twice")
        out[name] = value
    return out


def main(argv: Optional[List[str]] = None) -> None:
    ap = argparse.ArgumentParser(prog="predict", description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="saved model (.pt)")
    ap.add_argument("--fasta", required=True, help="input sequences")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--outputs", default=",".join(DEFAULT_OUTPUTS),
                    help=f"comma-separated subset of {','.join(OUTPUTS)}")
    ap.add_argument("--go-top-k", type=int, default=10)
    ap.add_argument("--attention-top-k", type=int, default=10,
                    help="positions per block and head of the attention_top output")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--truncate", action="store_true", help="keep the first L - 2 residues of longer sequences")
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is a GPU, else cpu")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])
    ap.add_argument("--head", action="append", default=[], metavar="NAME=PATH",
                    help="a fine-tuned head file (cli finetune) to predict with; adds the output task:NAME")
    ap.add_argument("--head-classes", action="append", default=[], metavar="NAME=ALPHABET",
                    help="class letters of a residue head (default: the head file's), for task_NAME_string")
    a = ap.parse_args(argv)
    device = torch.device(a.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    outputs = [o for o in a.outputs.split(",") if o]
    head_paths = _pairs(a.head, "--head")
    alphabets = _pairs(a.head_classes, "--head-classes")
    for name in alphabets:
        if name not in head_paths:
            raise SystemExit(f"--head-classes {name}=...: no --head of that name")
    outputs += [f"task:{name}" for name in head_paths if f"task:{name}" not in outputs]
    model = load_model(a.model, device=device, backend=a.backend)
    fa = FastaIndex(a.fasta)
    try:
        ids, seqs = [], []
        for name, seq in fa:
            ids.append(name)
            seqs.append(seq)
    finally:
        fa.close()
    pred = Predictor(model, batch_size=a.batch_size, device=device, heads=head_paths)
    for name, head in pred.heads.items():
        residue = isinstance(head, ProteinBERTForTokenClassification)
        if name not in alphabets and residue and (pred.head_meta[name] or {}).get("classes"):
            alphabets[name] = pred.head_meta[name]["classes"]
        if name in alphabets and not residue:
            raise SystemExit(f"--head-classes {name}: only a residue head has a class alphabet")
        if name in alphabets and len(alphabets[name]) != head.n_classes:
            raise SystemExit(f"head {name!r}: alphabet {alphabets[name]!r} has {len(alphabets[name])} letters, "
                             f"the head {head.n_classes} classes")
    res = pred.predict(seqs, outputs=outputs, go_top_k=a.go_top_k, truncate=a.truncate,
                       attention_top_k=a.attention_top_k)
    arrays = {k: (v.float() if v.dtype == torch.bfloat16 else v).numpy() for k, v in res.items()}
    L = model.sequences_length
    for name, alphabet in alphabets.items():
        # position 0 is <sos>: residue i of a record sits at i + 1, and a record holds min(len, L - 2) residues
        letters = np.array(list(alphabet))
        lab = arrays[f"task_{name}_labels"]
        arrays[f"task_{name}_string"] = np.array(
            ["".join(letters[lab[n, 1:1 + min(len(seq), L - 2)]]) for n, seq in enumerate(seqs)])
    np.savez(a.out, ids=np.array(ids), **arrays)
    print(json.dumps({"records": len(ids), "out": a.out, "arrays": sorted(arrays)}))


if __name__ == "__main__":
    main()
