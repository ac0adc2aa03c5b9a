"""``predict``: embeddings, GO-term predictions and residue calls for the records of a FASTA file.

    python -m proteinbert_pytorch_replication_amd.cli predict --model model.pt --fasta in.fasta --out out.npz \\
        [--outputs global,pooled,go_topk] [--go-top-k K] [--batch-size N] [--truncate]

The model is a file written by ``train.checkpoint.save_final_model`` (or a training checkpoint holding the
model's config); the ``.npz`` holds ``ids`` (the FASTA record names, in file order) and the arrays of the
requested outputs (:mod:`..inference`).  bf16 arrays are stored as fp32.  For a reference-semantics model
the residue probabilities and calls depend on ``--batch-size`` (see :mod:`..inference`).
"""
from __future__ import annotations

import argparse
import json
from typing import List, Optional

import numpy as np
import torch

from ..etl.fasta import FastaIndex
from ..inference import DEFAULT_OUTPUTS, OUTPUTS, Predictor
from ..train.checkpoint import load_model


def main(argv: Optional[List[str]] = None) -> None:
    ap = argparse.ArgumentParser(prog="predict", description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="saved model (.pt)")
    ap.add_argument("--fasta", required=True, help="input sequences")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--outputs", default=",".join(DEFAULT_OUTPUTS),
                    help=f"comma-separated subset of {','.join(OUTPUTS)}")
    ap.add_argument("--go-top-k", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--truncate", action="store_true", help="keep the first L - 2 residues of longer sequences")
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is a GPU, else cpu")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])
    a = ap.parse_args(argv)
    device = torch.device(a.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    outputs = [o for o in a.outputs.split(",") if o]
    model = load_model(a.model, device=device, backend=a.backend)
    fa = FastaIndex(a.fasta)
    try:
        ids, seqs = [], []
        for name, seq in fa:
            ids.append(name)
            seqs.append(seq)
    finally:
        fa.close()
    pred = Predictor(model, batch_size=a.batch_size, device=device)
    res = pred.predict(seqs, outputs=outputs, go_top_k=a.go_top_k, truncate=a.truncate)
    arrays = {k: (v.float() if v.dtype == torch.bfloat16 else v).numpy() for k, v in res.items()}
    np.savez(a.out, ids=np.array(ids), **arrays)
    print(json.dumps({"records": len(ids), "out": a.out, "arrays": sorted(arrays)}))


if __name__ == "__main__":
    main()
