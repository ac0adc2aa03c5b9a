"""Top-k neighbour search over a database of n = 1,048,576 embedded proteins (bf16 rows), the two forms alternated
in one process round by round, device events, medians of the rounds:

  (A) the torch form a user would write: per chunk of 65,536 database rows the bf16 ``q @ x[c].T``, ``torch.topk``
      of the chunk's scores, and a running merge (``cat`` with the kept candidates, ``topk`` again).  It rounds
      scores to bf16 and has no tie rule;
  (B) ``ops.search.search_topk``: one ``pbx_search_topk`` launch (32 x 32 score tiles on the bf16 MFMA, fp32
      scores, each query's best k kept as the database streams by) and the exact merge of the splits.

D = 512 and 128, nq = 1, 32 and 2048, k = 10 and 64.  For nq <= 32 the stream rate of X (n D 2 bytes per call) in
TB/s, for nq = 2048 the MFMA rate (2 nq n D flop per call) in PF/s; for nq = 2048 also the other grid order
(``order=0``: the query tile, not the split, varies fastest) and other split counts.  Before anything is timed the
forms are compared: the fraction of (A)'s neighbours that (B) returns too (they differ where bf16 rounding of the
scores reorders near-ties).  Last, the accuracy record of tests/test_hip_search.py: the worst |value - fp64| / tol.

    python tools/search_bench.py [--rounds 7] [--out profiles/r21/search_topk.txt]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteinbert_pytorch_replication_amd.ops.search import default_splits, search_topk  # noqa: E402

CHUNK = 65536
F64 = torch.float64


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def torch_form(q, x, k):
    run_v = run_i = None
    for c0 in range(0, x.shape[0], CHUNK):
        s = q @ x[c0:c0 + CHUNK].t()                              # bf16 GEMM, bf16 scores
        v, i = torch.topk(s, min(k, s.shape[1]), dim=1)
        i = i + c0
        if run_v is None:
            run_v, run_i = v, i
        else:
            cv, ci = torch.cat([run_v, v], dim=1), torch.cat([run_i, i], dim=1)
            run_v, pos = torch.topk(cv, k, dim=1)
            run_i = ci.gather(1, pos)
    return run_v, run_i


def unit_rows(n, D, gen):
    x = torch.randn(n, D, device="cuda", generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)


def shape_bench(x, nq, k, rounds, gen):
    n, D = x.shape
    q = unit_rows(nq, D, gen)
    reps = 1 if nq > 32 else 5
    fns = {"A_torch": lambda: torch_form(q, x, k), "B_fused": lambda: search_topk(q, x, k)}
    S = default_splits(nq, n, k, x.device)
    if nq > 32:
        fns["B_fused_query_tile_fastest"] = lambda: search_topk(q, x, k, order=0)
        fns["B_fused_half_splits"] = lambda: search_topk(q, x, k, splits=max(1, S // 2))
        fns["B_fused_twice_splits"] = lambda: search_topk(q, x, k, splits=min(2 * S, 16384 // k))
    for f in fns.values():                                        # warm-up: code objects, allocator
        f()
    torch.cuda.synchronize()
    (_, ia), (_, ib) = fns["A_torch"](), fns["B_fused"]()
    both = [len(set(a) & set(b)) / k for a, b in zip(ia.tolist(), ib.tolist())]
    us = {name: [] for name in fns}
    for _ in range(rounds):
        for name, f in fns.items():
            us[name].append(event_us(f, reps))
    med = {name: statistics.median(v) for name, v in us.items()}
    rec = {"n": n, "D": D, "nq": nq, "k": k, "splits": S, "overlap_A_B": round(sum(both) / len(both), 4),
           "us": {name: {"median": round(med[name], 1), "rounds": [round(t, 1) for t in v]} for name, v in us.items()},
           "B_over_A": round(med["B_fused"] / med["A_torch"], 3),
           "B_not_slower_than_A": bool(med["B_fused"] <= med["A_torch"])}
    if nq <= 32:
        rec["B_stream_TB_s"] = round(n * D * 2 / med["B_fused"] / 1e6, 3)
        rec["A_stream_TB_s"] = round(n * D * 2 / med["A_torch"] / 1e6, 3)
    else:
        rec["B_mfma_PF_s"] = round(2.0 * nq * n * D / med["B_fused"] / 1e9, 4)
        rec["A_gemm_PF_s"] = round(2.0 * nq * n * D / med["A_torch"] / 1e9, 4)
    return rec


def accuracy_record():
    """The rule of tests/test_hip_search.py at its shapes: fp64 scores of the same bf16 rows, e = max(error of an
    independent fp32 torch evaluation, 2^-24 max|s|), tol = 16 e."""
    worst = {"value_over_tol": 0.0, "unreturned_margin_over_2tol": 0.0}
    shapes = [(1, 1, 16, 1), (5, 33, 16, 5), (33, 95, 48, 32), (70, 1000, 128, 10), (40, 4133, 512, 64),
              (3, 2500, 1024, 64), (129, 300, 32, 7), (5, 100, 64, 64)]
    for nq, n, D, k in shapes:
        g = torch.Generator().manual_seed(nq * 7919 + n * 31 + D)
        q, x = torch.randn(nq, D, generator=g), torch.randn(n, D, generator=g)
        q = (q / q.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        x = (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        s64 = q.to(F64) @ x.to(F64).t()
        e = max(float(((q.float() @ x.float().t()).to(F64) - s64).abs().max()), 2.0 ** -24 * float(s64.abs().max()))
        tol = 16 * e
        for S in (1, 3, (n + 31) // 32 + 2):
            v, i = search_topk(q.cuda(), x.cuda(), k, splits=S)
            v, i = v.cpu(), i.cpu().long()
            rest = s64.clone()
            rest.scatter_(1, i, float("-inf"))
            margin = float((rest.max(1).values - v.to(F64).min(1).values).clamp(min=0).max()) if n > k else 0.0
            worst["value_over_tol"] = max(worst["value_over_tol"], float((v.to(F64) - s64.gather(1, i)).abs().max()) / tol)
            worst["unreturned_margin_over_2tol"] = max(worst["unreturned_margin_over_2tol"], margin / (2 * tol))
    return {"accuracy": {"shapes": shapes, "worst": {k: round(v, 4) for k, v in worst.items()}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1048576)
    ap.add_argument("--dims", default="512,128")
    ap.add_argument("--queries", default="1,32,2048")
    ap.add_argument("--ks", default="10,64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("search_bench: needs a GPU (no CPU fallback: a CPU time says nothing here)")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:                                                 # rewritten after every part: a partial run keeps them
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit({"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "chunk": CHUNK,
          "cus": torch.cuda.get_device_properties(0).multi_processor_count})
    gen = torch.Generator(device="cuda").manual_seed(0)
    for D in [int(v) for v in a.dims.split(",") if v]:
        x = unit_rows(a.rows, D, gen)
        for nq in [int(v) for v in a.queries.split(",") if v]:
            for k in [int(v) for v in a.ks.split(",") if v]:
                emit(shape_bench(x, nq, k, a.rounds, gen))
        del x
    emit(accuracy_record())


if __name__ == "__main__":
    main()
