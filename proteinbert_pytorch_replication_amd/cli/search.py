"""``index`` and ``search``: an embedding index of a FASTA file, and its nearest neighbours for another.

    python -m proteinbert_pytorch_replication_amd.cli index --model model.pt --fasta db.fasta --out db.npz \\
        [--embedding global|pooled] [--metric cosine|dot] [--batch-size N] [--truncate] [--device D] [--backend B]
    python -m proteinbert_pytorch_replication_amd.cli search --model model.pt --index db.npz --fasta q.fasta \\
        --k 10 --out hits.tsv [--batch-size N] [--truncate] [--device D] [--backend B]

``index`` embeds every record with the model (:class:`..inference.Predictor`) and writes the
:class:`..search.EmbeddingIndex` file; ``search`` embeds the query records the same way and writes one line per
hit, tab-separated: ``query_id``, ``rank`` (0 is the best), ``hit_id``, ``score``.  Both print a one-line JSON
summary.  Hits are exact: score descending, equal scores in the order of the database file.
"""
from __future__ import annotations

import argparse
import json
from typing import List, Optional, Tuple

import torch

from ..etl.fasta import FastaIndex
from ..inference import Predictor
from ..search import EMBEDDINGS, METRICS, EmbeddingIndex
from ..train.checkpoint import load_model


def _records(path: str) -> Tuple[List[str], List[str]]:
    fa = FastaIndex(path)
    try:
        ids, seqs = [], []
        for name, seq in fa:
            ids.append(name)
            seqs.append(seq)
    finally:
        fa.close()
    return ids, seqs


def _common(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("--model", required=True, help="saved model (.pt)")
    ap.add_argument("--fasta", required=True, help="input sequences")
    ap.add_argument("--batch-size", type=int, default=256, help="sequences per encoder pass")
    ap.add_argument("--truncate", action="store_true", help="keep the first L - 2 residues of longer sequences")
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is a GPU, else cpu")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])


def _predictor(a) -> Predictor:
    device = torch.device(a.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
    model = load_model(a.model, device=device, backend=a.backend)
    return Predictor(model, batch_size=a.batch_size, device=device)


def index_main(argv: Optional[List[str]] = None) -> None:
    ap = argparse.ArgumentParser(prog="index", description="embedding index of the records of a FASTA file")
    _common(ap)
    ap.add_argument("--out", required=True, help="output index (.npz)")
    ap.add_argument("--embedding", default="global", choices=list(EMBEDDINGS))
    ap.add_argument("--metric", default="cosine", choices=list(METRICS))
    a = ap.parse_args(argv)
    pred = _predictor(a)
    ids, seqs = _records(a.fasta)
    index = EmbeddingIndex.from_sequences(pred, seqs, ids=ids, embedding=a.embedding, metric=a.metric,
                                          truncate=a.truncate)
    index.save(a.out)
    print(json.dumps({"records": len(index), "dim": index.dim, "embedding": index.embedding,
                      "metric": index.metric, "out": a.out}))


def search_main(argv: Optional[List[str]] = None) -> None:
    ap = argparse.ArgumentParser(prog="search", description="nearest neighbours of FASTA records in an index")
    _common(ap)
    ap.add_argument("--index", required=True, help="index written by `index` (.npz)")
    ap.add_argument("--k", type=int, default=10, help="hits per query")
    ap.add_argument("--out", required=True, help="output hits (.tsv)")
    a = ap.parse_args(argv)
    pred = _predictor(a)
    index = EmbeddingIndex.load(a.index, device=pred.device, model=pred.model)
    if not 1 <= a.k <= len(index):
        raise SystemExit(f"--k {a.k}: the index holds {len(index)} records")
    ids, seqs = _records(a.fasta)
    hits = index.search_sequences(pred, seqs, k=a.k, truncate=a.truncate)
    with open(a.out, "w") as fh:
        for qid, names, scores in zip(ids, hits["ids"], hits["scores"].tolist()):
            for rank, (name, score) in enumerate(zip(names, scores)):
                fh.write(f"{qid}\t{rank}\t{name}\t{score:.9g}\n")
    print(json.dumps({"queries": len(ids), "k": a.k, "index_records": len(index), "embedding": index.embedding,
                      "metric": index.metric, "out": a.out}))
