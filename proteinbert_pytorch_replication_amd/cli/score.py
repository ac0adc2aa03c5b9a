"""``score``: pseudo-log-likelihoods, variant-effect scores and mutational scans for the records of a FASTA file.

    python -m proteinbert_pytorch_replication_amd.cli score --model model.pt --fasta in.fasta --out out.tsv \\
        [--variants variants.tsv] [--strategy wt_marginal|pll_ratio] [--scan] [--batch-size N] [--truncate] \\
        [--device D] [--backend auto|hip|torch]

The output is a tab-separated table with a header line:

* default: one line per record: ``id``, ``n_residues``, ``pll``, ``pseudo_perplexity`` (``exp(-pll /
  n_residues)``; ``nan`` for a record without residues);
* ``--scan``: one line per record, position and letter: ``id``, ``pos`` (1-based), ``wt``, ``mut``, ``llr``: the
  log-odds of every substitution (the 22 letters of the vocabulary) at every residue;
* ``--variants FILE``: ``FILE`` holds ``id<TAB>variant`` lines (``A123G``, or ``A123G:L45P`` for several
  substitutions; lines that are empty or start with ``#`` are skipped); one line per variant: ``id``,
  ``variant``, ``score``, by ``--strategy`` (:meth:`..inference.Predictor.score_variants`).  An id that the
  FASTA file does not hold is an error.

The scores are functions of the local head's logits under a softmax over the vocabulary, in both semantics (see
:mod:`..inference`), and do not depend on ``--batch-size``.
"""
from __future__ import annotations

import argparse
import json
import math
from typing import Dict, List, Optional, Tuple

import torch

from ..etl.fasta import FastaIndex
from ..inference import SCORE_STRATEGIES, Predictor
from ..train.checkpoint import load_model


def _read_variants(path: str) -> List[Tuple[str, str]]:
    rows = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            cols = line.split("\t")
            if len(cols) != 2 or not cols[0] or not cols[1]:
                raise SystemExit(f"{path}:{n}: expected id<TAB>variant")
            rows.append((cols[0], cols[1]))
    return rows


def main(argv: Optional[List[str]] = None) -> None:
    ap = argparse.ArgumentParser(prog="score", description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="saved model (.pt)")
    ap.add_argument("--fasta", required=True, help="input sequences")
    ap.add_argument("--out", required=True, help="output .tsv")
    ap.add_argument("--variants", default=None, help="TSV of id<TAB>variant to score (e.g. A123G, A123G:L45P)")
    ap.add_argument("--strategy", default="wt_marginal", choices=list(SCORE_STRATEGIES))
    ap.add_argument("--scan", action="store_true", help="every substitution at every residue of every record")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--truncate", action="store_true", help="keep the first L - 2 residues of longer sequences")
    ap.add_argument("--device", default=None, help="default: cuda:0 when there is a GPU, else cpu")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"])
    a = ap.parse_args(argv)
    if a.scan and a.variants:
        raise SystemExit("--scan and --variants are two tables: run them one at a time")
    device = torch.device(a.device or ("cuda:0" if torch.cuda.is_available() else "cpu"))
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
    lines = 0
    if a.variants:
        by_id: Dict[str, str] = dict(zip(ids, seqs))
        rows = _read_variants(a.variants)
        wanted: Dict[str, List[str]] = {}
        for rid, variant in rows:
            if rid not in by_id:
                raise SystemExit(f"{a.variants}: id {rid!r} is not in {a.fasta}")
            wanted.setdefault(rid, []).append(variant)
        # one score_variants call per record (one wild-type pass each), written in the file's order
        scores = {rid: iter(pred.score_variants(by_id[rid], variants, strategy=a.strategy,
                                                truncate=a.truncate)["scores"].tolist())
                  for rid, variants in wanted.items()}
        with open(a.out, "w") as out:
            out.write("id\tvariant\tscore\n")
            for rid, variant in rows:
                out.write(f"{rid}\t{variant}\t{next(scores[rid]):.9g}\n")
                lines += 1
        mode = "variants"
    elif a.scan:
        with open(a.out, "w") as out:
            out.write("id\tpos\twt\tmut\tllr\n")
            for rid, seq in zip(ids, seqs):
                scan = pred.mutation_scan(seq, truncate=a.truncate)
                for p, row in enumerate(scan["llr"].tolist()):
                    for mut, v in zip(scan["letters"], row):
                        out.write(f"{rid}\t{p + 1}\t{seq[p]}\t{mut}\t{v:.9g}\n")
                        lines += 1
        mode = "scan"
    else:
        res = pred.predict(seqs, outputs=("pll",), truncate=a.truncate)
        with open(a.out, "w") as out:
            out.write("id\tn_residues\tpll\tpseudo_perplexity\n")
            for rid, n, pll in zip(ids, res["n_residues"].tolist(), res["pll"].tolist()):
                ppl = math.exp(-pll / n) if n > 0 else float("nan")
                out.write(f"{rid}\t{n}\t{pll:.9g}\t{ppl:.9g}\n")
                lines += 1
        mode = "pll"
    print(json.dumps({"records": len(ids), "out": a.out, "mode": mode, "lines": lines}))


if __name__ == "__main__":
    main()
